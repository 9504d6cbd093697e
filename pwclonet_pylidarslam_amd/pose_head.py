"""The training pose head as hand-written kernels each way (csrc/pose_head_train.hip).

``pose_head_train(emb, logits, w_qt, b_qt, w_q, b_q, w_t, b_t, state, rank, head)`` is PW/pose_calculator.py:47-86 in
``train()`` mode, from the mask LOGITS (the soft-max over the points is part of it): value and gradients of the torch
ops it replaces up to fp32 rounding, with the two dropout masks drawn from the counter-based generator that
``training.DropoutStream`` owns -- keep bit = a function of (seed, step, rank, head, branch, cloud, unit), the same on any
device and in every replay of a captured graph.  A kept value is doubled, a dropped one is zero (``F.dropout`` at p = 0.5).

Saved for backward: the inputs, the row maximum and reciprocal sum of the soft-max, the pooled vector, the hidden vector,
the keep bytes and the un-normalised quaternion; backward never reads the stream's state, so several forwards before a
backward stay correct.  ``reference(...)`` is the same formula in torch ops under given masks (CPU tensors, other
dtypes: tests and the float64 yardstick).
"""
import torch
import torch.nn.functional as F
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib

IN_CHANNELS, HIDDEN = 64, 256


def supported(emb, logits, weights=()):
    """Whether the kernels cover these tensors: fp32 (B, 64, N) on the GPU, N >= 1, fp32 parameters of the head's shapes."""
    ok = (emb.is_cuda and logits.is_cuda and emb.dtype == torch.float32 and logits.dtype == torch.float32
          and emb.dim() == 3 and emb.shape == logits.shape and emb.shape[1] == IN_CHANNELS and emb.shape[0] >= 1
          and emb.shape[2] >= 1 and emb.numel() < (1 << 38))
    if ok and weights:
        shapes = ((HIDDEN, IN_CHANNELS), (HIDDEN,), (4, HIDDEN), (4,), (3, HIDDEN), (3,))
        ok = len(weights) == 6 and all(w.is_cuda and w.dtype == torch.float32 and w.numel() == s[0] * (s[1] if len(s) > 1 else 1)
                                       and w.is_contiguous() and w.data_ptr() % 16 == 0 for w, s in zip(weights, shapes))
    return bool(ok)


def _aligned(t):
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


class _PoseHeadTrain(Function):
    @staticmethod
    def forward(ctx, emb, logits, w_qt, b_qt, w_q, b_q, w_t, b_t, state, rank, head, keep_log):
        e, x = _aligned(emb), _aligned(logits)
        B, _, N = e.shape
        dev = e.device
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        rowmax, rinv, pooled = f32(B, IN_CHANNELS), f32(B, IN_CHANNELS), f32(B, IN_CHANNELS)
        big, q_raw, q, t = f32(B, HIDDEN), f32(B, 4), f32(B, 4), f32(B, 3)
        keep = torch.empty((B, HIDDEN), dtype=torch.uint8, device=dev)
        _lib.call("pose_head_train_forward_kernel_wrapper", dev, B, N, e.data_ptr(), x.data_ptr(), w_qt.data_ptr(),
                  b_qt.data_ptr(), w_q.data_ptr(), b_q.data_ptr(), w_t.data_ptr(), b_t.data_ptr(), state.data_ptr(),
                  int(rank), int(head), rowmax.data_ptr(), rinv.data_ptr(), pooled.data_ptr(), big.data_ptr(),
                  keep.data_ptr(), None if keep_log is None else keep_log.data_ptr(), q_raw.data_ptr(), q.data_ptr(),
                  t.data_ptr())
        ctx.save_for_backward(e, x, w_qt, w_q, w_t, rowmax, rinv, pooled, big, keep, q_raw)
        ctx.shapes = tuple(w.shape for w in (w_qt, b_qt, w_q, b_q, w_t, b_t))
        ctx.mark_non_differentiable(keep)
        return q, t, keep

    @staticmethod
    @once_differentiable
    def backward(ctx, g_q, g_t, _g_keep):
        e, x, w_qt, w_q, w_t, rowmax, rinv, pooled, big, keep, q_raw = ctx.saved_tensors
        B, _, N = e.shape
        dev = e.device
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        g_q = torch.zeros_like(q_raw) if g_q is None else g_q.contiguous()
        g_t = f32(B, 3).zero_() if g_t is None else g_t.contiguous()
        g_qraw, g_big, g_pooled = f32(B, 4), f32(B, HIDDEN), f32(B, IN_CHANNELS)
        d_emb, d_logits = torch.empty_like(e), torch.empty_like(x)
        grads = [f32(*s) for s in ctx.shapes]
        _lib.call("pose_head_train_backward_kernel_wrapper", dev, B, N, e.data_ptr(), x.data_ptr(), w_qt.data_ptr(),
                  w_q.data_ptr(), w_t.data_ptr(), rowmax.data_ptr(), rinv.data_ptr(), pooled.data_ptr(), big.data_ptr(),
                  keep.data_ptr(), q_raw.data_ptr(), g_q.data_ptr(), g_t.data_ptr(), g_qraw.data_ptr(), g_big.data_ptr(),
                  g_pooled.data_ptr(), d_emb.data_ptr(), d_logits.data_ptr(), *[g.data_ptr() for g in grads])
        return (d_emb, d_logits, *grads, None, None, None, None)


def pose_head_train(emb, logits, w_qt, b_qt, w_q, b_q, w_t, b_t, state, rank=0, head=0, keep_log=None):
    """(emb, logits (B,64,N); the head's six parameters; state (3,) i64 on the device = {seed, next step, step in flight})
    -> (q (B,4) normalised, t (B,3), keep (B,256) u8: bit 0 = the q branch kept the unit, bit 1 = the t branch).
    Reads the seed and the step in flight from ``state`` on the device.  ``keep_log``: a (B,256) u8 tensor that receives
    the keep bytes as well.  There is no fall-back: tensors the kernels do not cover are an error (``supported``)."""
    weights = (w_qt, b_qt, w_q, b_q, w_t, b_t)
    if not supported(emb, logits, weights):
        raise RuntimeError("pose_head_train: needs float32 (B, 64, N) tensors and the head's float32 parameters on the GPU, "
                           "got emb %s %s on %s" % (emb.dtype, tuple(emb.shape), emb.device))
    if state.dtype != torch.int64 or state.numel() != 3 or state.device != emb.device:
        raise RuntimeError("pose_head_train: state must be (3,) int64 on the tensors' device")
    if not 0 <= int(rank) < (1 << 28) or not 0 <= int(head) < 4:
        raise ValueError("pose_head_train: rank=%r outside [0, 2^28) or head=%r outside 0..3" % (rank, head))
    if keep_log is not None and (keep_log.dtype != torch.uint8 or tuple(keep_log.shape) != (emb.shape[0], HIDDEN)
                                 or not keep_log.is_contiguous() or keep_log.device != emb.device):
        raise RuntimeError("pose_head_train: keep_log must be contiguous uint8 (B, 256) on the tensors' device")
    return _PoseHeadTrain.apply(emb, logits, *weights, state, rank, head, keep_log)


def reference(emb, logits, w_qt, b_qt, w_q, b_q, w_t, b_t, keep_q, keep_t, scale=2.0):
    """The same head in torch ops (any device and dtype) under given masks keep_q / keep_t (B,256) bool:
    -> (q (B,4) normalised, t (B,3))."""
    pooled = torch.sum(emb * F.softmax(logits, dim=2), dim=2)
    big = F.linear(pooled, w_qt.reshape(HIDDEN, IN_CHANNELS), b_qt)
    big_q = big * (keep_q.to(big.dtype) * scale)
    big_t = big * (keep_t.to(big.dtype) * scale)
    q = F.linear(big_q, w_q.reshape(4, HIDDEN), b_q)
    q = q / (torch.sqrt(torch.sum(q * q, dim=1, keepdim=True) + 1e-10) + 1e-10)
    t = F.linear(big_t, w_t.reshape(3, HIDDEN), b_t)
    return q, t
