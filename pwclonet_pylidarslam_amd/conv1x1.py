"""Pointwise convolution of the module path's shared MLPs on the HIP kernels of ``csrc/conv1x1.hip`` (SURVEY.md
section 8 row f3): forward, input gradient and weight gradient on the fp32 matrix cores, on the ``(B, C, S, K)``
channel-major activations as they are (no NHWC transposes).

``conv1x1(x, weight)`` has the semantics of ``torch.nn.functional.conv{1,2,3}d(x, weight)`` for a kernel of size 1,
stride 1, no padding, no bias (P2/pytorch_utils.py:114-167 builds exactly these inside SharedMLP); anything else
stays on torch (``supported`` says which).  The three products are fp32 FMAs, so results equal torch's up to
summation order; the weight gradient is summed in a fixed order (deterministic).
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib


import os as _os

# BatchNorm-backward sums in the input-gradient epilogue (conv1x1_dgrad_bnstats): OPT-IN.  Built and tested (VERDICT r2 item
# 5 (ii)), measured neutral: graphed step 24.67 / 24.96 ms with, 24.75 / 24.76 without -- the reduction pass it removes reads
# bn_x and da at the HBM rate, the epilogue that replaces it reads bn_x in a kernel that is HBM-bound at those (few-channel,
# long-row) shapes as well, plus seven vector instructions per element on the pipe the MFMA needs.
_DGRAD_SUMS = _os.environ.get("PWCLO_DGRAD_SUMS", "0") != "0"


def _shape(x, weight):
    B, Cin = x.shape[0], x.shape[1]
    return B, Cin, weight.shape[0], x.numel() // max(B * Cin, 1)


def _aligned(t):
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def _fits(cin, cout):
    nbi, nbo = -(-cin // 16), -(-cout // 16)
    gy = -(-nbo // 8)
    return nbi * (-(-nbo // gy)) <= 150                      # KiB of LDS for the packed weights


def supported_layer(conv, batch, pixels, ndim):
    """``supported`` for an input described by its batch size, pixels per (batch, channel) row and rank only -- for
    callers that check a whole stack before running its first layer."""
    if not (isinstance(conv, (torch.nn.Conv1d, torch.nn.Conv2d, torch.nn.Conv3d)) and conv.weight.dtype == torch.float32
            and conv.bias is None and conv.groups == 1 and conv.padding_mode == "zeros"):
        return False
    if any(k != 1 for k in conv.kernel_size) or any(s != 1 for s in conv.stride) or any(d != 1 for d in conv.dilation):
        return False
    if isinstance(conv.padding, str) or any(p != 0 for p in conv.padding):
        return False
    if ndim != conv.weight.dim() or batch <= 0 or pixels <= 0:
        return False
    cin, cout, P = conv.in_channels, conv.out_channels, pixels
    if P % 4 != 0 or cin > 512 or cout > 512 or batch * (-(-P // 64)) >= 2 ** 31:
        return False
    if 4 * batch * max(cin, cout) * P >= 2 ** 32 - 16:        # the kernels address x (forward) / dy (input gradient) with
        return False                                          # 32-bit byte offsets through a buffer descriptor
    # weight gradient: double-buffered 32-pixel chunks of all cin + cout rows in LDS, 7 float4 of staging per thread
    return (_fits(cin, cout) and _fits(cout, cin) and 2 * (cin + cout) * 36 * 4 <= 150 * 1024
            and (cin + cout) * 8 <= 7 * 512 and _wgrad_split(cin, cout))


def supported(x, conv):
    """True when ``conv(x)`` is a bias-free pointwise convolution these kernels cover (forward and both gradients)."""
    if not (isinstance(conv, (torch.nn.Conv1d, torch.nn.Conv2d, torch.nn.Conv3d)) and x.is_cuda
            and x.dtype == torch.float32 and x.dim() >= 3 and x.shape[1] == conv.in_channels and x.numel() > 0):
        return False
    return supported_layer(conv, x.shape[0], x.numel() // (x.shape[0] * conv.in_channels), x.dim())


def _wgrad_split(cin, cout):
    """csrc/conv1x1.hip wgrad_plan: the 8 waves split into wo x wm workers over the (cout/16, cin/16) tile grid, each
    owning at most 4 x 4 tiles (fewer than 5 tiles: one tile per worker, pixels split instead)."""
    nbo, nbi = -(-cout // 16), -(-cin // 16)
    if nbo * nbi < 5:
        return True
    return any(-(-nbo // wo) <= 4 and -(-nbi // (8 // wo)) <= 4 for wo in (1, 2, 4, 8))


PLAN_KINDS = {"forward": 0, "dgrad": 1, "stats": 2, "dgrad_sums": 3, "affine": 4, "pooled": 5, "wgrad": 6}   # PWCLO_PLAN_*
_PLAN_FIELDS = (("nbo", "gy", "gx", "lean", "stats"), ("ro", "rm", "ph", "wo", "wm", "cp", "grid"))


def plan(kind, b, cin, cout, p, cus=0):
    """conv1x1_plan_query: the kernel instantiation and grid the entry point ``kind`` (a key of ``PLAN_KINDS``) selects
    for the sizes as that entry point takes them -> dict of the fields documented in include/pwclo_ops.h plus
    ``accepted`` (False: the launcher refuses the shape).  ``cus`` > 0 stands in for the device's CU count; the call is
    then host-only and works without a GPU."""
    import ctypes
    out = (ctypes.c_int * 8)()
    rc = _lib.load().conv1x1_plan_query(PLAN_KINDS[kind], b, cin, cout, p, cus, out)
    if rc < 0:
        raise ValueError("conv1x1_plan_query(%s, %d, %d, %d, %d, %d)" % (kind, b, cin, cout, p, cus))
    fields = _PLAN_FIELDS[kind == "wgrad"]
    return dict(zip(fields, out[:len(fields)]), accepted=rc == 0)


def _forward(x, w2d, transposed, cin, cout):
    B = x.shape[0]
    P = x.numel() // (B * cin)
    y = torch.empty((B, cout) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
    _lib.call("conv1x1_forward_kernel_wrapper", x.device, B, cin, cout, P, x.data_ptr(), w2d.data_ptr(),
              int(transposed), y.data_ptr())
    return y


def _conv_backward(ctx, dy):
    x, weight = ctx.saved_tensors
    dy = _aligned(dy)
    w = _aligned(weight.detach())
    B, cin, cout, P = _shape(x, w)
    dx = dw = None
    if ctx.needs_input_grad[0]:
        dx = _forward(dy, w, True, cout, cin)                     # dX = W^T dY: same kernel, transposed view
    if ctx.needs_input_grad[1]:
        nbytes = _lib.load().conv1x1_wgrad_workspace_bytes(B, cin, cout, P)
        ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=x.device)
        dw = torch.empty_like(w)
        _lib.call("conv1x1_wgrad_kernel_wrapper", x.device, B, cin, cout, P, dy.data_ptr(), x.data_ptr(),
                  dw.data_ptr(), ws.data_ptr())
        dw = dw.view_as(weight)
    return dx, dw


class _Conv1x1(Function):
    @staticmethod
    def forward(ctx, x, weight):
        x = _aligned(x)
        w = _aligned(weight.detach())
        B, cin, cout, P = _shape(x, w)
        ctx.save_for_backward(x, weight)
        return _forward(x, w, False, cin, cout)

    @staticmethod
    @once_differentiable            # raw kernels: a second differentiation raises instead of returning constants
    def backward(ctx, dy):
        return _conv_backward(ctx, dy)


def conv1x1(x, weight):
    """``F.conv{1,2,3}d(x, weight)`` for a size-1 kernel: x (B, Cin, *), weight (Cout, Cin, 1[, 1[, 1]])."""
    return _Conv1x1.apply(x, weight)


def _forward_stats(x, w, cin, cout, in_tf, rm, rv, momentum, eps):
    """The convolution (optionally with the previous BatchNorm + ReLU applied on load, ``in_tf = (mean, invstd, gamma,
    beta)``) that also leaves the batch statistics of its OUTPUT: (y, mean, invstd) and the running-statistics update."""
    B = x.shape[0]
    P = x.numel() // (B * cin)
    y = torch.empty((B, cout) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
    mean = torch.empty((cout,), dtype=torch.float32, device=x.device)
    invstd = torch.empty((cout,), dtype=torch.float32, device=x.device)
    nbytes = _lib.load().conv1x1_stats_workspace_bytes(B, cin, cout, P)
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=x.device)
    p = lambda t: t.data_ptr() if t is not None else 0
    tf = in_tf if in_tf is not None else (None, None, None, None)
    from . import batchnorm as hb
    name, mom = hb._momentum_entry("conv1x1_forward_bnstats_kernel_wrapper", momentum)
    _lib.call(name, x.device, B, cin, cout, P, p(x), p(w), p(tf[0]), p(tf[1]), p(tf[2]), p(tf[3]), p(y), float(eps), mom,
              p(rm), p(rv), p(mean), p(invstd), p(ws))
    return y, mean, invstd


class _Conv1x1Stats(Function):
    """``_Conv1x1`` whose forward also returns the batch statistics (mean, 1/sqrt(var + eps)) of its output, summed in the
    convolution's epilogue, for the training-mode BatchNorm that follows it (and updates that layer's running
    statistics).  The statistics are returned as constants: the consumer's backward (batchnorm / _BNReluConv) is the full
    BatchNorm backward, which already accounts for their dependence on the output."""

    @staticmethod
    def forward(ctx, x, weight, running_mean, running_var, momentum, eps):
        x = _aligned(x)
        w = _aligned(weight.detach())
        B, cin, cout, P = _shape(x, w)
        ctx.save_for_backward(x, weight)
        y, mean, invstd = _forward_stats(x, w, cin, cout, None, running_mean, running_var, momentum, eps)
        ctx.mark_non_differentiable(mean, invstd)
        ctx.set_materialize_grads(False)          # no zero-filled "gradients" of the two statistics vectors in backward
        return y, mean, invstd

    @staticmethod
    @once_differentiable
    def backward(ctx, dy, _dmean, _dinvstd):
        if dy is None:
            return None, None, None, None, None, None
        dx, dw = _conv_backward(ctx, dy)
        return dx, dw, None, None, None, None


def _bn_buffers(bn):
    rm = bn.running_mean if bn.track_running_stats else None
    rv = bn.running_var if bn.track_running_stats else None
    return rm, rv


def conv1x1_stats(x, conv, bn):
    """``conv(x)`` plus the batch statistics of the result for the training-mode module ``bn`` that follows ``conv`` in
    its block: -> (y, (mean, invstd)); ``bn``'s running statistics and counter are updated as ``bn(y)`` would."""
    from . import batchnorm as hb
    momentum = hb.momentum_of(bn, x)
    hb.count_batch(bn)
    rm, rv = _bn_buffers(bn)
    y, mean, invstd = _Conv1x1Stats.apply(x, conv.weight, rm, rv, momentum, bn.eps)
    touch_running_stats(rm, rv)
    return y, (mean, invstd)


def _folded(bn):
    """Per-channel (scale, shift) of an eval-mode BatchNorm, cached on the module until one of its tensors changes
    (version counters) or moves: a handful of tiny kernels once, not per call.  The training kernels write the running
    statistics through raw pointers; they bump the version counters themselves (``touch_running_stats``), and
    ``pytorch_utils._BN.train()`` drops the cache on every train() / eval() switch, which also covers statistics
    written by a hipGraph replay of a training step (no Python runs then)."""
    tensors = (bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.num_batches_tracked)
    key = tuple((t.data_ptr(), t._version) if t is not None else None for t in tensors) + (bn.eps,)
    cached = getattr(bn, "_pwclo_folded", None)
    if cached is not None and cached[0] == key:
        return cached[1], cached[2]
    with torch.no_grad():
        scale = torch.rsqrt(bn.running_var.float() + bn.eps)
        if bn.weight is not None:
            scale = scale * bn.weight.float()
        shift = -bn.running_mean.float() * scale
        if bn.bias is not None:
            shift = shift + bn.bias.float()
        scale, shift = scale.contiguous(), shift.contiguous()
    object.__setattr__(bn, "_pwclo_folded", (key, scale, shift))
    return scale, shift


def touch_running_stats(*tensors):
    """Make a raw-pointer write to BatchNorm buffers visible to torch's version tracking (the folded eval
    cache keyed on ``_version`` went stale after a training-mode forward that no optimizer step followed)."""
    for t in tensors:
        if t is not None:
            torch.autograd.graph.increment_version(t)


def conv1x1_bn_eval(x, conv, bn, relu):
    """Eval-mode ``act(bn(conv(x)))`` of a conv -> BatchNorm [-> ReLU] block as ONE kernel (no autograd): the running
    statistics folded to a per-channel scale / shift in the convolution's epilogue.  Same values as the three modules up
    to fp32 rounding of the folded affine map."""
    x = _aligned(x)
    w = _aligned(conv.weight.detach())
    B, cin, cout, P = _shape(x, w)
    scale, shift = _folded(bn)
    y = torch.empty((B, cout) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
    _lib.call("conv1x1_affine_forward_kernel_wrapper", x.device, B, cin, cout, P, x.data_ptr(), w.data_ptr(),
              scale.data_ptr(), shift.data_ptr(), int(bool(relu)), y.data_ptr())
    return y


def conv1x1_bn_eval_maxk(x, conv, bn, relu):
    """``act(bn(conv(x))).max(dim=3)[0]`` for x (B, Cin, S, K), K in {4, 8, 16, 32}, eval mode, no autograd: one
    kernel, the (B, Cout, S, K) activation is never written."""
    x = _aligned(x)
    w = _aligned(conv.weight.detach())
    B, cin, S, K = x.shape
    cout = w.shape[0]
    scale, shift = _folded(bn)
    pooled = torch.empty((B, cout, S), dtype=torch.float32, device=x.device)
    _lib.call("conv1x1_affine_maxk_forward_kernel_wrapper", x.device, B, cin, cout, S, K, x.data_ptr(), w.data_ptr(),
              scale.data_ptr(), shift.data_ptr(), int(bool(relu)), pooled.data_ptr())
    return pooled


class _BNReluConv(Function):
    """Interior layer of a training-mode stack as ONE autograd node: BatchNorm (batch statistics) + ReLU of the previous
    convolution's output ``x`` fused into this layer's convolution -- statistics pass, then the convolution applies the
    normalisation while loading (the normalised activation is never written).  Backward: weight gradient on the same
    transformed input, input gradient of the convolution, then the BatchNorm + ReLU backward on ``x`` (its ReLU mask is
    recomputed from ``x`` like in batchnorm._BatchNormTrain)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum, eps, weight, given_mean=None, given_invstd=None,
                out_stats=None):
        """``given_*``: the batch statistics of x from the producing convolution's epilogue (no statistics pass here).
        ``out_stats = (running_mean, running_var, momentum, eps)`` of the BatchNorm FOLLOWING this convolution: the
        forward then returns (y, mean_y, invstd_y) like ``_Conv1x1Stats``."""
        from . import batchnorm as hb
        x = _aligned(x)
        w = _aligned(weight.detach())
        B, cin, cout, P = _shape(x, w)
        p = lambda t: t.data_ptr() if t is not None else 0
        if given_mean is not None:
            mean, invstd = given_mean, given_invstd
        else:
            mean = torch.empty((cin,), dtype=torch.float32, device=x.device)
            invstd = torch.empty((cin,), dtype=torch.float32, device=x.device)
            ws = hb._workspace(cin, x.device)
            name, mom = hb._momentum_entry("batchnorm_train_forward_kernel_wrapper", momentum)
            _lib.call(name, x.device, B, cin, P, p(x), p(gamma), p(beta), float(eps), mom, p(running_mean),
                      p(running_var), 0, p(mean), p(invstd), p(ws), 1)
        ctx.save_for_backward(x, gamma, beta, mean, invstd, weight)
        if out_stats is not None:
            y, mean_y, invstd_y = _forward_stats(x, w, cin, cout, (mean, invstd, gamma, beta), *out_stats)
            ctx.mark_non_differentiable(mean_y, invstd_y)
            ctx.set_materialize_grads(False)
            return y, mean_y, invstd_y
        y = torch.empty((B, cout) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
        _lib.call("conv1x1_bnrelu_forward_kernel_wrapper", x.device, B, cin, cout, P, p(x), p(w), p(mean), p(invstd),
                  p(gamma), p(beta), p(y))
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy, *_dstats):
        from . import batchnorm as hb
        if dy is None:
            return (None,) * 11
        x, gamma, beta, mean, invstd, weight = ctx.saved_tensors
        dy = _aligned(dy)
        w = _aligned(weight.detach())
        B, cin, cout, P = _shape(x, w)
        p = lambda t: t.data_ptr() if t is not None else 0
        dw = None
        if ctx.needs_input_grad[7]:
            nbytes = _lib.load().conv1x1_wgrad_workspace_bytes(B, cin, cout, P)
            ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=x.device)
            dw = torch.empty_like(w)
            _lib.call("conv1x1_bnrelu_wgrad_kernel_wrapper", x.device, B, cin, cout, P, p(dy), p(x), p(mean), p(invstd),
                      p(gamma), p(beta), p(dw), p(ws))
            dw = dw.view_as(weight)
        dx = dgamma = dbeta = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dx = torch.empty_like(x)
            dgamma = torch.empty((cin,), dtype=torch.float32, device=x.device)
            dbeta = torch.empty((cin,), dtype=torch.float32, device=x.device)
            if _DGRAD_SUMS and cin <= 64:         # (wider: the epilogue's registers do not fit; those tensors are small)
                # the BatchNorm backward's two sums come out of the input-gradient convolution's epilogue (one read of da
                # less); then the apply pass alone
                da = torch.empty_like(x)
                nbytes = _lib.load().conv1x1_stats_workspace_bytes(B, cout, cin, P)
                ws2 = torch.empty((nbytes // 8,), dtype=torch.float64, device=x.device)
                _lib.call("conv1x1_dgrad_bnstats_kernel_wrapper", x.device, B, cin, cout, P, p(dy), p(w), p(x), p(mean),
                          p(invstd), p(gamma), p(beta), p(da), p(dgamma), p(dbeta), p(ws2))
                _lib.call("batchnorm_train_backward_apply_kernel_wrapper", x.device, B, cin, P, p(x), p(da), p(gamma), p(beta),
                          p(mean), p(invstd), p(dgamma), p(dbeta), p(dx), 1)
            else:
                da = _forward(dy, w, True, cout, cin)                 # gradient w.r.t. the normalised, rectified input
                ws2 = hb._workspace(cin, x.device)
                _lib.call("batchnorm_train_backward_kernel_wrapper", x.device, B, cin, P, p(x), p(da), p(gamma), p(beta),
                          p(mean), p(invstd), p(dx), p(dgamma), p(dbeta), p(ws2), 1)
            if gamma is None:
                dgamma = dbeta = None
        return dx, dgamma, dbeta, None, None, None, None, dw, None, None, None


def bn_relu_conv(x, bn, conv, stats=None, next_bn=None):
    """``conv(relu(bn(x)))`` for a training-mode ``torch.nn.BatchNorm*`` module ``bn`` (updates its running statistics and
    ``num_batches_tracked`` like ``bn(x)``) and a bias-free pointwise ``conv`` that ``supported(x, conv)`` accepts.
    ``stats``: (mean, invstd) of ``x`` when the convolution that produced ``x`` already summed them (``conv1x1_stats`` /
    this function with ``next_bn``; the running statistics were updated there).  ``next_bn``: the training-mode BatchNorm
    that follows ``conv``; the result is then (y, (mean_y, invstd_y)) and ``next_bn``'s buffers are updated."""
    from . import batchnorm as hb
    momentum = hb.momentum_of(bn, x) if stats is None else bn.momentum        # (with stats given it is not used)
    next_momentum = hb.momentum_of(next_bn, x) if next_bn is not None else None
    if stats is None:
        hb.count_batch(bn)
        rm, rv = _bn_buffers(bn)
    else:
        rm = rv = None
    given = stats if stats is not None else (None, None)
    out_stats = None
    if next_bn is not None:
        hb.count_batch(next_bn)
        nrm, nrv = _bn_buffers(next_bn)
        out_stats = (nrm, nrv, next_momentum, next_bn.eps)
    out = _BNReluConv.apply(x, bn.weight, bn.bias, rm, rv, momentum, bn.eps, conv.weight, given[0], given[1], out_stats)
    touch_running_stats(rm, rv)
    if next_bn is not None:
        touch_running_stats(nrm, nrv)
        return out[0], (out[1], out[2])
    return out
