"""Every csrc/conv1x1.hip instantiation the host dispatch can select -- conv1x1_kernel<NBO, STATS, LEAN> through its six
entry points, conv1x1_wgrad_kernel<RO, RM, XF> in every rectangle and pixel-phase form -- each at the smallest ragged
shape that selects it, against a float64 evaluation of the same operation on the same fp32 inputs.

One table (tests/conv_variant_cases.py; tests/test_conv_plan_cpu.py proves on the CPU that it reaches every form the
dispatch can select on 256 CUs), one test per row.  A row calls the C entry point itself through ``_lib.call``, after
asserting through conv1x1_plan_query -- with the device's own CU count -- that its shape selects the form it names, so a
change of the dispatch cannot quietly move the rows back to NBO = 1.

Criteria (``pytest -s`` prints every figure and, at the end, the worst ratio per family):

* convolution values (y, da, dw, and the outputs of the folded-BatchNorm / ReLU / max-over-K epilogue): the max-abs
  error against float64 is at most 4 x E32, the max-abs error of the same expression evaluated by torch in fp32 on the
  CPU (the yardstick of tests/test_gpu_stack_variants.py: the margin covers the other summation order), and at most
  1e-5 of the tensor's scale.
* the statistics epilogue (STATS = 1): y bit-identical to the plain kernel's; mean within 2e-6 of |mean| + std, invstd
  within 5e-6 relative, running statistics rtol 1e-5 / atol 1e-6, all against float64 statistics of that y.
* the BatchNorm-backward sums (STATS = 2): da bit-identical to the plain input gradient; dgamma, dbeta and dx (after
  batchnorm_train_backward_apply) within 1e-5 of each tensor's scale of a float64 BatchNorm + ReLU backward evaluated
  from the same da, mean and invstd.  A layer of more than 64 channels is refused with a library error, da untouched.
* ReLU masks are decided in fp32 by the kernels and in float64 by the references: the inputs are built so that no
  pre-activation lies within 1e-4 of zero (asserted), which makes the two masks identical by construction.

Outputs of 4 GiB and more (the general epilogue with 64-bit addresses for a plain forward) are out of scope here: no
case allocates more than a few hundred MB.
"""
import math

import pytest
import torch

import conv_variant_cases as T

pytestmark = pytest.mark.gpu

MARGIN, CAP, RELU_GAP = 4.0, 1e-5, 1e-4
EPS, MOMENTUM = 1e-5, 0.1
_WORST = {}


def _p(t):
    return t.data_ptr() if t is not None else 0


def _gen(case):
    return torch.Generator().manual_seed(1000003 * case.cin + 1009 * case.cout + case.p + 7 * len(case.opts))


def _call(name, dev, *args):
    from pwclonet_pylidarslam_amd import _lib
    _lib.call(name, dev, *args)


def _select(case):
    """The form the device's own dispatch selects must be the one the row names."""
    from pwclonet_pylidarslam_amd import conv1x1
    plan = conv1x1.plan(case.entry, case.b, case.cin, case.cout, case.p)
    if case.entry == "wgrad":
        got = (plan["ro"], plan["rm"], plan["ph"])
    else:
        got = (plan["nbo"], plan["gy"], plan["lean"], plan["stats"])
    assert got == case.want, "%s: the device's dispatch selects %s" % (T.case_id(case), plan)
    assert plan["accepted"] != bool(case.opts.get("refused")), plan
    return plan


def _values(family, case, got, ref64, cpu32):
    """The convolution criterion: max-abs error <= 4 x E32 and <= 1e-5 of the scale."""
    assert bool(torch.isfinite(got).all())
    err = (got.double() - ref64).abs().max().item()
    e32 = (cpu32.to(ref64.device).double() - ref64).abs().max().item()
    scale = ref64.abs().max().item()
    ratio = err / e32 if e32 > 0 else (0.0 if err == 0 else math.inf)
    print("\n%s [%s]: scale %.3g  E32 %.3e  kernel %.3e (%.2f x E32, %.2e of the scale)"
          % (T.case_id(case), family, scale, e32, err, ratio, err / scale))
    if ratio > _WORST.get(family, (-1.0, ""))[0]:
        _WORST[family] = (ratio, T.case_id(case))
    assert err <= MARGIN * e32, "%s %s: max error %.3e > 4 x E32 = %.3e" % (T.case_id(case), family, err, MARGIN * e32)
    assert err <= CAP * scale, "%s %s: max error %.3e > 1e-5 of the scale %.3g" % (T.case_id(case), family, err, scale)


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios():
    yield
    for family in sorted(_WORST):
        print("\nworst error / E32 of %-12s %.2f  (%s)" % (family + ":", _WORST[family][0], _WORST[family][1]))


def _layer(case, g, dev):
    x = torch.randn(case.b, case.cin, case.p, generator=g).to(dev)
    w = (torch.randn(case.cout, case.cin, generator=g) / case.cin ** 0.5).to(dev)
    return x, w


def _transform(cin, g, dev):
    """(mean, invstd, gamma, beta) of a BatchNorm in front of the layer."""
    return tuple(t.to(dev) for t in (torch.randn(cin, generator=g) * 0.5, torch.rand(cin, generator=g) + 0.5,
                                     torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.3))


def _bn(x, tf):
    """The kernels' expression ((x - mean) * invstd) * gamma + beta in x's own type (gamma / beta may be None)."""
    mean, invstd, gamma, beta = (None if t is None else t.to(x.dtype).view(1, -1, 1) for t in tf)
    h = (x - mean) * invstd
    if gamma is not None:
        h = h * gamma
    return h if beta is None else h + beta


def _settle_elements(x, tf):
    """Move the few elements of x whose BatchNorm output lies within RELU_GAP of zero (0.01 in x is at least 2.5e-3 there:
    invstd and gamma are >= 0.5), then assert that none is left."""
    near = _bn(x.double(), tf).abs() < RELU_GAP
    x[near] += 0.01
    assert not bool((_bn(x.double(), tf).abs() < RELU_GAP).any())
    return int(near.sum())


def _settle_columns(x, pre, g):
    """Redraw the pixels of x (whole channel columns) at which any output channel's pre-activation ``pre(x)`` (float64)
    lies within RELU_GAP of zero, until none does; asserted."""
    moved = 0
    for _ in range(10):
        near = (pre(x).abs() < RELU_GAP).any(dim=1)                 # (b, p)
        n = int(near.sum())
        if n == 0:
            break
        moved += n
        x.permute(0, 2, 1)[near] = torch.randn(n, x.shape[1], generator=g).to(x.device)
    assert not bool((pre(x).abs() < RELU_GAP).any())
    return moved


def _conv64(x, w):
    return torch.einsum("oi,bip->bop", w.double(), x.double())


def _plain_forward(case, dev, x, w, transposed=0):
    b, p = case.b, case.p
    cin, cout = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
    y = torch.empty(b, cout, p, device=dev)
    _call("conv1x1_forward_kernel_wrapper", dev, b, cin, cout, p, _p(x), _p(w), transposed, _p(y))
    return y


# ---- the six entry points of the forward family, the weight gradient -------------------------------------------------

def run_forward(case, dev):
    x, w = _layer(case, _gen(case), dev)
    y = _plain_forward(case, dev, x, w)
    _values("forward", case, y, _conv64(x, w), torch.matmul(w.cpu(), x.cpu()))


def run_dgrad(case, dev):
    g = _gen(case)
    dy = torch.randn(case.b, case.cout, case.p, generator=g).to(dev)
    w = (torch.randn(case.cout, case.cin, generator=g) / case.cin ** 0.5).to(dev)
    da = _plain_forward(case, dev, dy, w, transposed=1)
    assert da.shape == (case.b, case.cin, case.p)
    ref = torch.einsum("oi,bop->bip", w.double(), dy.double())
    _values("dgrad", case, da, ref, torch.matmul(w.cpu().t(), dy.cpu()))


def run_affine(case, dev):
    """conv1x1_affine_forward / conv1x1_affine_maxk_forward: conv -> y * scale + shift -> [ReLU] -> [max over k]."""
    g = _gen(case)
    b, cin, cout, p, k, relu = case.b, case.cin, case.cout, case.p, case.opts.get("k", 0), case.opts["relu"]
    x, w = _layer(case, g, dev)
    sign = torch.where(torch.rand(cout, generator=g) < 0.25, -1.0, 1.0)
    scale = ((torch.rand(cout, generator=g) + 0.5) * sign).to(dev)
    shift = (torch.randn(cout, generator=g) * 0.5).to(dev)
    pre = lambda t: _conv64(t, w) * scale.double().view(1, -1, 1) + shift.double().view(1, -1, 1)
    if relu:
        print("\n%s: %d pixels redrawn" % (T.case_id(case), _settle_columns(x, pre, g)))

    def finish(z):
        z = torch.relu(z) if relu else z
        return z.view(b, cout, p // k, k).amax(dim=3) if k else z
    ref = finish(pre(x))
    cpu = finish(torch.matmul(w.cpu(), x.cpu()) * scale.cpu().view(1, -1, 1) + shift.cpu().view(1, -1, 1))
    if k:
        out = torch.empty(b, cout, p // k, device=dev)
        _call("conv1x1_affine_maxk_forward_kernel_wrapper", dev, b, cin, cout, p // k, k, _p(x), _p(w), _p(scale), _p(shift),
              relu, _p(out))
    else:
        out = torch.empty(b, cout, p, device=dev)
        _call("conv1x1_affine_forward_kernel_wrapper", dev, b, cin, cout, p, _p(x), _p(w), _p(scale), _p(shift), relu, _p(out))
    _values("pooled" if k else "affine", case, out, ref, cpu)


def run_stats(case, dev):
    from pwclonet_pylidarslam_amd import _lib
    g = _gen(case)
    b, cin, cout, p = case.b, case.cin, case.cout, case.p
    x, w = _layer(case, g, dev)
    sigmas = case.opts.get("mean_sigmas")
    if sigmas:                         # x + u with W u = sigmas x |W row|: every channel's mean is `sigmas` of its deviations
        u = torch.linalg.pinv(w.double()) @ (sigmas * w.double().norm(dim=1))
        x += u.float().view(1, -1, 1)
    tf = None
    if case.opts["transform"]:
        tf = _transform(cin, g, dev)
        print("\n%s: %d elements moved" % (T.case_id(case), _settle_elements(x, tf)))
    rm, rv = torch.randn(cout, generator=g).to(dev), (torch.rand(cout, generator=g) + 0.5).to(dev)
    rm0, rv0 = rm.clone(), rv.clone()
    y, mean, invstd = torch.empty(b, cout, p, device=dev), torch.empty(cout, device=dev), torch.empty(cout, device=dev)
    ws = torch.empty((_lib.load().conv1x1_stats_workspace_bytes(b, cin, cout, p) // 8,), dtype=torch.float64, device=dev)
    t4 = tf or (None,) * 4
    _call("conv1x1_forward_bnstats_kernel_wrapper", dev, b, cin, cout, p, _p(x), _p(w), _p(t4[0]), _p(t4[1]), _p(t4[2]),
          _p(t4[3]), _p(y), EPS, MOMENTUM, _p(rm), _p(rv), _p(mean), _p(invstd), _p(ws))
    if tf:
        plain = torch.empty_like(y)
        _call("conv1x1_bnrelu_forward_kernel_wrapper", dev, b, cin, cout, p, _p(x), _p(w), _p(tf[0]), _p(tf[1]), _p(tf[2]),
              _p(tf[3]), _p(plain))
        a32 = torch.relu(_bn(x.cpu(), tuple(t.cpu() for t in tf)))
        _values("transform", case, plain, _conv64(torch.relu(_bn(x.double(), tf)), w), torch.matmul(w.cpu(), a32))
    else:
        plain = _plain_forward(case, dev, x, w)
    assert torch.equal(y, plain), "y differs from the plain kernel's"
    y64 = y.double()
    m64, v64 = y64.mean(dim=(0, 2)), y64.var(dim=(0, 2), unbiased=False)
    sd = v64.sqrt()
    if sigmas:
        assert bool((m64.abs() >= (sigmas - 1) * sd).all()), (m64.abs() / sd).min().item()
    e_mean = ((mean.double() - m64).abs() / (m64.abs() + sd)).max().item()
    is64 = 1.0 / torch.sqrt(v64 + EPS)
    e_inv = ((invstd.double() - is64).abs() / is64).max().item()
    print("\n%s: mean %.2e of |mean| + std (bound 2e-6), invstd %.2e relative (bound 5e-6), max |mean| / std %.1f"
          % (T.case_id(case), e_mean, e_inv, (m64.abs() / sd).max().item()))
    assert ((mean.double() - m64).abs() <= 2e-6 * (m64.abs() + sd) + 1e-12).all(), e_mean
    assert e_inv <= 5e-6, e_inv
    n = b * p
    torch.testing.assert_close(rm.double(), (1 - MOMENTUM) * rm0.double() + MOMENTUM * m64, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(rv.double(), (1 - MOMENTUM) * rv0.double() + MOMENTUM * v64 * n / (n - 1), rtol=1e-5,
                               atol=1e-6)


def run_dgrad_sums(case, dev):
    from pwclonet_pylidarslam_amd import _lib
    g = _gen(case)
    b, cin, cout, p = case.b, case.cin, case.cout, case.p
    x = (torch.randn(b, cin, p, generator=g) * 2 + 0.5).to(dev)                  # the BatchNorm's input
    dy = torch.randn(b, cout, p, generator=g).to(dev)
    w = (torch.randn(cout, cin, generator=g) / cin ** 0.5).to(dev)
    mean = x.double().mean(dim=(0, 2)).float()
    invstd = (1.0 / torch.sqrt(x.double().var(dim=(0, 2), unbiased=False) + EPS)).float()
    affine = case.opts["affine"]
    gamma = (torch.rand(cin, generator=g) + 0.5).to(dev) if affine else None
    beta = (torch.randn(cin, generator=g) * 0.3).to(dev) if affine else None
    tf = (mean, invstd, gamma, beta)
    _settle_elements(x, tf)
    da = torch.full((b, cin, p), 7.0, device=dev)
    dgamma, dbeta = torch.full((cin,), 7.0, device=dev), torch.full((cin,), 7.0, device=dev)
    ws = torch.empty((_lib.load().conv1x1_stats_workspace_bytes(b, cout, cin, p) // 8,), dtype=torch.float64, device=dev)
    args = (b, cin, cout, p, _p(dy), _p(w), _p(x), _p(mean), _p(invstd), _p(gamma), _p(beta), _p(da), _p(dgamma), _p(dbeta),
            _p(ws))
    if case.opts.get("refused"):
        with pytest.raises(RuntimeError, match="conv1x1_dgrad_bnstats"):
            _call("conv1x1_dgrad_bnstats_kernel_wrapper", dev, *args)
        _lib.synchronize(dev)
        assert bool((da == 7.0).all()) and bool((dgamma == 7.0).all()) and bool((dbeta == 7.0).all())
        return
    _call("conv1x1_dgrad_bnstats_kernel_wrapper", dev, *args)
    dx = torch.empty_like(x)
    _call("batchnorm_train_backward_apply_kernel_wrapper", dev, b, cin, p, _p(x), _p(da), _p(gamma), _p(beta), _p(mean),
          _p(invstd), _p(dgamma), _p(dbeta), _p(dx), 1)
    assert torch.equal(da, _plain_forward(case, dev, dy, w, transposed=1)), "da differs from the plain input gradient"
    xh = (x.double() - mean.double().view(1, -1, 1)) * invstd.double().view(1, -1, 1)
    gm = da.double() * (_bn(x.double(), tf) > 0)
    r_dbeta, r_dgamma = gm.sum(dim=(0, 2)), (gm * xh).sum(dim=(0, 2))
    m = b * p
    g64 = gamma.double() if affine else torch.ones(cin, dtype=torch.float64, device=dev)
    r_dx = (gm - (r_dbeta / m).view(1, -1, 1) - xh * (r_dgamma / m).view(1, -1, 1)) * (g64 * invstd.double()).view(1, -1, 1)
    for got, ref, what in ((dgamma, r_dgamma, "dgamma"), (dbeta, r_dbeta, "dbeta"), (dx, r_dx, "dx")):
        scale, err = ref.abs().max().item(), (got.double() - ref).abs().max().item()
        print("\n%s %s: %.2e of the scale (bound 1e-5)" % (T.case_id(case), what, err / scale))
        assert err <= 1e-5 * scale, (what, err, scale)


def run_wgrad(case, dev):
    from pwclonet_pylidarslam_amd import _lib
    g = _gen(case)
    b, cin, cout, p, xf = case.b, case.cin, case.cout, case.p, case.opts["xf"]
    x = torch.randn(b, cin, p, generator=g).to(dev)
    dy = torch.randn(b, cout, p, generator=g).to(dev)
    ws = torch.empty((_lib.load().conv1x1_wgrad_workspace_bytes(b, cin, cout, p) // 4,), device=dev)
    dw = torch.empty(cout, cin, device=dev)
    flat = lambda t: t.permute(1, 0, 2).reshape(t.shape[1], -1)
    if xf:
        tf = _transform(cin, g, dev)
        _settle_elements(x, tf)
        _call("conv1x1_bnrelu_wgrad_kernel_wrapper", dev, b, cin, cout, p, _p(dy), _p(x), _p(tf[0]), _p(tf[1]), _p(tf[2]),
              _p(tf[3]), _p(dw), _p(ws))
        a64, a32 = torch.relu(_bn(x.double(), tf)), torch.relu(_bn(x.cpu(), tuple(t.cpu() for t in tf)))
    else:
        _call("conv1x1_wgrad_kernel_wrapper", dev, b, cin, cout, p, _p(dy), _p(x), _p(dw), _p(ws))
        a64, a32 = x.double(), x.cpu()
    ref = torch.einsum("bop,bip->oi", dy.double(), a64)
    _values("wgrad xf" if xf else "wgrad", case, dw, ref, flat(dy.cpu()) @ flat(a32).t())


RUN = dict(forward=run_forward, dgrad=run_dgrad, affine=run_affine, pooled=run_affine, stats=run_stats,
           dgrad_sums=run_dgrad_sums, wgrad=run_wgrad)


@pytest.mark.parametrize("case", T.CASES, ids=[T.case_id(c) for c in T.CASES])
def test_conv1x1_variant_against_float64(cuda, case):
    _select(case)
    RUN[case.entry](case, cuda)
