"""Every kernel instantiation and entry point of csrc/batchnorm.hip, and every K of csrc/softmax_wsum.hip, against float64.

The cases, inputs, references and bounds are those of tests/bn_cases.py; tests/test_bn_plan_cpu.py proves (without a GPU)
that they reach every form the launchers select, that the exact cases are exact and that the bounds are neither vacuous nor
loose.  The C entry points are called by name through ``_lib.call``:
  dense cases     batchnorm_train_forward, _backward, _apply, _backward_apply (statistics (a), element-wise passes (b))
  devmom          batchnorm_train_forward_devmom, batchnorm_train_relu_maxk_forward_devmom: the argument form's bits
  exact cases     batchnorm_train_relu_maxk_apply, _relu_maxk_backward, _apply, _backward_apply, _backward: torch.equal (c)
  max-K cases     batchnorm_train_relu_maxk_forward, _relu_maxk_backward against the dense path (d)
  refusals        what the host rejects before any launch (e)
  softmax         softmax_wsum forward / backward, K in {1, 2, 4, 6, 8, 16, 32}
Run with -s for the largest observed error of each check family as a fraction of its bound.
"""
import pytest
import torch

import bn_cases as T

pytestmark = pytest.mark.gpu

RATIOS = {}


def _within(what, got, want, bound, ok=None):
    """|got - want| <= bound element-wise (``ok``: elements excused); records the largest error / bound."""
    err = (got.double().cpu() - want).abs()
    bad = err > bound
    if ok is not None:
        bad = bad & ~ok
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double())
    if ok is not None:
        ratio = ratio[~ok]
    if ratio.numel():
        RATIOS[what] = max(RATIOS.get(what, 0.0), float(ratio.max()))
    assert not bool(bad.any()), (what, float(ratio.max()) if ratio.numel() else 0.0)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(RATIOS):
        print("\nlargest error / bound  %-28s %.4f" % (k, RATIOS[k]), end="")
    print()


def P(t):
    return t.data_ptr() if t is not None else 0


def _call(name, dev, *args):
    from pwclonet_pylidarslam_amd import _lib
    _lib.call(name + "_kernel_wrapper", dev, *args)


def _ws(c, dev):
    from pwclonet_pylidarslam_amd import _lib
    return torch.empty((_lib.load().batchnorm_train_workspace_bytes(c) // 8,), dtype=torch.float64, device=dev)


def _dev(t, dev):
    return t.to(dev) if t is not None else None


def _forward(dev, x, g, be, rm, rv, relu, entry="batchnorm_train_forward", momentum=T.MOMENTUM):
    b, c, L = x.shape
    y = torch.empty_like(x)
    sm, si = torch.empty(c, device=dev), torch.empty(c, device=dev)
    _call(entry, dev, b, c, L, P(x), P(g), P(be), T.EPS, momentum, P(rm), P(rv), P(y), P(sm), P(si), P(_ws(c, dev)), int(relu))
    return y, sm, si


def _backward(dev, x, dy, g, be, sm, si, relu):
    b, c, L = x.shape
    dx = torch.empty_like(x)
    dg, db = torch.empty(c, device=dev), torch.empty(c, device=dev)
    _call("batchnorm_train_backward", dev, b, c, L, P(x), P(dy), P(g), P(be), P(sm), P(si), P(dx), P(dg), P(db), P(_ws(c, dev)),
          int(relu))
    return dx, dg, db


def _apply(dev, x, g, be, mean, invstd, relu):
    b, c, L = x.shape
    y = torch.empty_like(x)
    _call("batchnorm_train_apply", dev, b, c, L, P(x), P(g), P(be), P(mean), P(invstd), P(y), int(relu))
    return y


def _backward_apply(dev, x, dy, g, be, sm, si, dg, db, relu):
    b, c, L = x.shape
    dx = torch.empty_like(x)
    _call("batchnorm_train_backward_apply", dev, b, c, L, P(x), P(dy), P(g), P(be), P(sm), P(si), P(dg), P(db), P(dx), int(relu))
    return dx


def _maxk_forward(dev, x, g, be, rm, rv, entry="batchnorm_train_relu_maxk_forward", momentum=T.MOMENTUM):
    b, c, S, K = x.shape
    pooled, xsel = torch.empty(b, c, S, device=dev), torch.empty(b, c, S, device=dev)
    arg = torch.empty(b, c, S, dtype=torch.uint8, device=dev)
    sm, si = torch.empty(c, device=dev), torch.empty(c, device=dev)
    _call(entry, dev, b, c, S, K, P(x), P(g), P(be), T.EPS, momentum, P(rm), P(rv), P(pooled), P(arg), P(xsel), P(sm), P(si),
          P(_ws(c, dev)))
    return pooled, arg, xsel, sm, si


def _maxk_apply(dev, x, g, be, mean, invstd):
    b, c, S, K = x.shape
    pooled, xsel = torch.empty(b, c, S, device=dev), torch.empty(b, c, S, device=dev)
    arg = torch.empty(b, c, S, dtype=torch.uint8, device=dev)
    _call("batchnorm_train_relu_maxk_apply", dev, b, c, S, K, P(x), P(g), P(be), P(mean), P(invstd), P(pooled), P(arg), P(xsel))
    return pooled, arg, xsel


def _maxk_backward(dev, x, dpool, arg, xsel, g, be, sm, si):
    b, c, S, K = x.shape
    dx = torch.empty_like(x)
    dg, db = torch.empty(c, device=dev), torch.empty(c, device=dev)
    _call("batchnorm_train_relu_maxk_backward", dev, b, c, S, K, P(x), P(dpool), P(arg), P(xsel), P(g), P(be), P(sm), P(si), P(dx),
          P(dg), P(db), P(_ws(c, dev)))
    return dx, dg, db


def _check_stats(tag, ref, sm, si, rm, rv, rm0, rv0):
    bm, bv, bi = T.stats_bounds(ref)
    _within("a.%s.mean" % tag, sm, ref["mean"], bm)
    _within("a.%s.invstd" % tag, si, ref["invstd"], bi)
    if rm is not None:
        wm, wv, brm, brv = T.running_reference(ref, rm0, rv0)
        _within("a.%s.running_mean" % tag, rm, wm, brm)
        _within("a.%s.running_var" % tag, rv, wv, brv)


def _check_backward(tag, xh, y64, by, dy64, mask_kernel, relu, si, g, dx, dg, db, M):
    """(b): dgamma / dbeta over the ReLU mask (the kernel's own decision where |y| is within its bound of zero), dx from the
    kernel's own sums.  -> the share of such elements."""
    amb = (y64.abs() <= by) if relu else None
    if relu:
        assert float(amb.double().mean()) <= 1e-4
        mask = torch.where(amb, mask_kernel, y64 > 0)
        gv = dy64 * mask
    else:
        gv = dy64
    wg, wb, bg, bb = T.sums_reference(xh.reshape(xh.shape[0], xh.shape[1], -1), gv.reshape(xh.shape[0], xh.shape[1], -1),
                                      (dy64.abs() * amb).reshape(xh.shape[0], xh.shape[1], -1) if relu else None)
    _within("b.%s.dbeta" % tag, db, wb, bb)
    _within("b.%s.dgamma" % tag, dg, wg, bg)
    c0, c1 = T.kernel_c01(dg.cpu(), db.cpu(), M)
    want, bound = T.backward_reference(xh, gv, si.cpu(), g, c0, c1)
    ok = None
    if relu and bool(amb.any()):                   # the other decision is a correct fp32 evaluation there too
        alt, balt = T.backward_reference(xh, torch.where(amb, dy64 - gv, gv), si.cpu(), g, c0, c1)
        ok = amb & ((dx.double().cpu() - alt).abs() <= balt)
    _within("b.%s.dx" % tag, dx, want, bound, ok)


@pytest.mark.parametrize("case", T.DENSE_CASES, ids=T.dense_id)
def test_dense_case_statistics_and_elementwise_passes(cuda, case):
    """(a) and (b) of one dense case: every family's statistics (repeated: the same bits), and on the Gaussian family the four
    configurations (relu, affine, running statistics) through forward / backward, with the given-statistics entry points
    giving the same bits."""
    b, c, L = case.b, case.c, case.L
    M = b * L
    rm0, rv0 = T.running_init(c)
    dy = T.dense_grad(case)
    dyd, dy64 = dy.to(cuda), dy.double()
    for family in T.FAMILIES:
        x = T.dense_input(case, family)
        xd = x.to(cuda)
        ref = T.stats_reference(x)
        for relu, affine, running in (T.CONFIGS if family == "gauss" else T.CONFIGS[:1]):
            tag = "%s" % family
            g, be = T.affine_params(c, affine)
            gd, bd = _dev(g, cuda), _dev(be, cuda)
            rm, rv = (rm0.to(cuda), rv0.to(cuda)) if running else (None, None)
            y, sm, si = _forward(cuda, xd, gd, bd, rm, rv, relu)
            _check_stats(tag, ref, sm, si, rm, rv, rm0, rv0)
            if family == "const":                  # var = 0 exactly in fp64 (3.25^2 sums exactly): the clamp, 1 / sqrt(eps)
                assert float(sm[0]) == 3.25 and abs(float(si[0]) - T.EPS ** -0.5) <= T.U * T.EPS ** -0.5
            rm2, rv2 = (rm0.to(cuda), rv0.to(cuda)) if running else (None, None)
            y2, sm2, si2 = _forward(cuda, xd, gd, bd, rm2, rv2, relu)
            assert torch.equal(sm, sm2) and torch.equal(si, si2) and torch.equal(y, y2)          # a fixed summation order
            assert not running or (torch.equal(rm, rm2) and torch.equal(rv, rv2))
            if family != "gauss":
                continue
            tag = "relu%d" % relu
            y64, by, xh = T.forward_reference(x, sm.cpu(), si.cpu(), g, be)
            _within("b.%s.y" % tag, y, y64.clamp_min(0.0) if relu else y64, by)
            assert torch.equal(_apply(cuda, xd, gd, bd, sm, si, relu), y)
            dx, dg, db = _backward(cuda, xd, dyd, gd, bd, sm, si, relu)
            dx2, dg2, db2 = _backward(cuda, xd, dyd, gd, bd, sm, si, relu)
            assert torch.equal(dg, dg2) and torch.equal(db, db2) and torch.equal(dx, dx2)
            assert torch.equal(_backward_apply(cuda, xd, dyd, gd, bd, sm, si, dg, db, relu), dx)
            _check_backward(tag, xh, y64, by, dy64, y.cpu() > 0, relu, si, g, dx, dg, db, M)


def test_devmom_entry_points_give_the_argument_forms_bits(cuda):
    """The momentum read from device memory: identical running statistics (and everything else) to the argument form."""
    case = T.Dense(9, 5, 1028, None, {})
    x = T.dense_input(case, "gauss").to(cuda)
    g, be = (t.to(cuda) for t in T.affine_params(5, 1))
    rm0, rv0 = T.running_init(5)
    mom = torch.full((1,), 0.3, device=cuda)
    outs = []
    for entry, m in (("batchnorm_train_forward", float(mom)), ("batchnorm_train_forward_devmom", P(mom))):
        rm, rv = rm0.to(cuda), rv0.to(cuda)
        outs.append(_forward(cuda, x, g, be, rm, rv, 1, entry=entry, momentum=m) + (rm, rv))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    assert not torch.equal(outs[0][3], rm0.to(cuda))
    x4 = x.reshape(9, 5, 257, 4)
    outs = []
    for entry, m in (("batchnorm_train_relu_maxk_forward", float(mom)), ("batchnorm_train_relu_maxk_forward_devmom", P(mom))):
        rm, rv = rm0.to(cuda), rv0.to(cuda)
        outs.append(_maxk_forward(cuda, x4, g, be, rm, rv, entry=entry, momentum=m) + (rm, rv))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    # without running statistics the cell is not needed
    _forward(cuda, x, g, be, None, None, 0, entry="batchnorm_train_forward_devmom", momentum=0)


@pytest.mark.parametrize("K", [4, 8, 16, 32])
def test_exact_boundary_and_tie_cases(cuda, K):
    """(c): mean = 0, invstd = 1, gamma in {1, -1, 0.5, 2, 0}, x multiples of 1/8, integer gradients: every value is exact in
    fp32, so the kernels must give the float64 reference's bits."""
    for b, S in ((2, 1024), (2, 4096 // K)):
        x, g, be, kinds, where = T.exact_maxk(K, b, S)
        C = x.shape[1]
        xd, gd, bd = x.to(cuda), g.to(cuda), be.to(cuda)
        zero, one = torch.zeros(C, device=cuda), torch.ones(C, device=cuda)
        y64, _, xh = T.forward_reference(x, zero.cpu(), one.cpu(), g, be)
        want_p, want_a, want_x = T.maxk_reference(x.double(), y64)
        pooled, arg, xsel = _maxk_apply(cuda, xd, gd, bd, zero, one)
        assert torch.equal(pooled.cpu(), want_p.float()) and torch.equal(arg.cpu(), want_a) and torch.equal(xsel.cpu(), want_x.float())
        y = _apply(cuda, xd.reshape(b, C, S * K), gd, bd, zero, one, 1)
        assert torch.equal(y.cpu(), y64.clamp_min(0.0).float().reshape(b, C, S * K))
        assert torch.equal(y.reshape(b, C, S, K).max(dim=3)[0], pooled)
        # what the rows were built for, on the kernel's own outputs
        a, p_, kd, live = arg.cpu(), pooled.cpu(), torch.from_numpy(kinds), g != 0
        for k_ in (T.KIND_UNIQUE, T.KIND_TIE):                        # the unique maximum at every position; a tie at i < j: i
            first = torch.from_numpy(where[kinds == k_, 0]).to(torch.uint8)
            assert bool((a[:, live][:, :, kd == k_] == first).all()) and bool((p_[:, live][:, :, kd == k_] > 0).all())
        for k_ in (T.KIND_ZERO, T.KIND_MINUS, T.KIND_NONPOS):         # nothing positive: pooled 0, arg 0
            assert bool((p_[:, live][:, :, kd == k_] == 0).all()) and bool((a[:, live][:, :, kd == k_] == 0).all())
        assert bool((p_[:, live][:, :, kd == T.KIND_PLUS] == (g[live].abs() / 8).reshape(1, -1, 1)).all())
        assert bool((a[:, ~live] == 0).all())                         # gamma = 0: the whole row ties
        neg = g < 0                                                   # negative gamma: the smallest x wins
        assert bool((xsel.cpu()[:, neg][p_[:, neg] > 0] == x[:, neg].min(dim=3)[0][p_[:, neg] > 0]).all())
        if b * S * K != 2 ** 13:
            continue
        dpool = T.exact_dpool(b, C, S, K)
        dx, dg, db = _maxk_backward(cuda, xd, dpool.to(cuda), arg, xsel, gd, bd, zero, one)
        # dbeta: the integer sum of dpool over the rows the forward left positive -- any disagreement between the forward's
        # ReLU and either backward mask changes it by an integer; gamma = 0 passes gradient only where beta > 0
        assert torch.equal(db.cpu(), (dpool * (p_ > 0)).sum(dim=(0, 2)))
        assert bool((db.cpu()[(g == 0) & (be <= 0)] == 0).all()) and bool((db.cpu()[(g == 0) & (be > 0)] == dpool[:, (g == 0) & (be > 0)].sum(dim=(0, 2))).all())
        dy = T.scatter_dpool(dpool.double(), want_a, want_p, K)
        wg, wb, _, _ = T.sums_reference(xh.reshape(b, C, -1), dy.reshape(b, C, -1))
        assert torch.equal(dg.cpu(), wg.float()) and torch.equal(db.cpu(), wb.float())
        c0, c1 = T.kernel_c01(dg.cpu(), db.cpu(), b * S * K)
        want_dx, _ = T.backward_reference(xh, dy, one.cpu(), g, c0, c1)
        assert torch.equal(dx.cpu(), want_dx.float())
        # the dense backward on the materialised sparse gradient: the same bits, from the given sums and from its own reduction
        dyd = dy.float().reshape(b, C, S * K).to(cuda)
        x3 = xd.reshape(b, C, S * K)
        assert torch.equal(_backward_apply(cuda, x3, dyd, gd, bd, zero, one, dg, db, 1).reshape(dx.shape), dx)
        dx3, dg3, db3 = _backward(cuda, x3, dyd, gd, bd, zero, one, 1)
        assert torch.equal(dg3, dg) and torch.equal(db3, db) and torch.equal(dx3.reshape(dx.shape), dx)


@pytest.mark.parametrize("case", T.MAXK_CASES, ids=T.maxk_id)
def test_maxk_case_against_the_dense_path(cuda, case):
    """(d): Gaussian rows with duplicated neighbours.  pooled is bit-equal to the max over K of batchnorm_train_forward(relu = 1)
    (same expression, same statistics), arg the first index attaining it, the gradients within the bounds of (b) for the
    gradient scattered to arg; with and without gamma / beta (and running statistics)."""
    b, c, S, K = case.b, case.c, case.S, case.K
    x, dpool = T.maxk_input(case)
    xd, dpd = x.to(cuda), dpool.to(cuda)
    ref = T.stats_reference(x.reshape(b, c, S * K))
    rm0, rv0 = T.running_init(c)
    for affine in (1, 0):
        g, be = T.affine_params(c, affine)
        gd, bd = _dev(g, cuda), _dev(be, cuda)
        rm, rv = (rm0.to(cuda), rv0.to(cuda)) if affine else (None, None)
        pooled, arg, xsel, sm, si = _maxk_forward(cuda, xd, gd, bd, rm, rv)
        _check_stats("maxk", ref, sm, si, rm, rv, rm0, rv0)
        y, sm2, si2 = _forward(cuda, xd.reshape(b, c, S * K), gd, bd, None, None, 1)
        assert torch.equal(sm, sm2) and torch.equal(si, si2)
        y4 = y.reshape(b, c, S, K).cpu()
        want_p = y4.max(dim=3)[0]
        want_a = (y4 == want_p.unsqueeze(3)).to(torch.uint8).argmax(dim=3).to(torch.uint8)
        assert torch.equal(pooled.cpu(), want_p) and torch.equal(arg.cpu(), want_a)
        assert torch.equal(xsel.cpu(), x.gather(3, want_a.long().unsqueeze(3)).squeeze(3))
        dx, dg, db = _maxk_backward(cuda, xd, dpd, arg, xsel, gd, bd, sm, si)
        y64, by, xh = T.forward_reference(x, sm.cpu(), si.cpu(), g, be)
        dy = T.scatter_dpool(dpool.double(), want_a, torch.ones_like(want_p), K)          # dpool at arg; the mask decides below
        _check_backward("maxk", xh, y64, by, dy, y4 > 0, 1, si, g, dx, dg, db, b * S * K)


def test_arguments_refused_before_any_launch(cuda):
    """(e): k outside {4, 8, 16, 32}, one of running_mean / running_var alone, a _devmom call with running statistics and no
    momentum pointer: the library error is set and the outputs keep what they held."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 8, 12, generator=g).to(cuda)
    c = 3
    ws = _ws(c, cuda)
    rm, rv = torch.zeros(c, device=cuda), torch.ones(c, device=cuda)
    mom = torch.full((1,), 0.1, device=cuda)
    mark = 7.5

    def outs():
        # every buffer large enough for any (s, k) below, should a refusal ever fail to refuse
        return dict(y=torch.full((2, 3, 96), mark, device=cuda), pooled=torch.full((2, 3, 96), mark, device=cuda),
                    arg=torch.full((2, 3, 96), 9, dtype=torch.uint8, device=cuda), xsel=torch.full((2, 3, 96), mark, device=cuda),
                    sm=torch.full((c,), mark, device=cuda), si=torch.full((c,), mark, device=cuda),
                    dx=torch.full((2, 3, 96), mark, device=cuda), dg=torch.full((c,), mark, device=cuda),
                    db=torch.full((c,), mark, device=cuda))

    def refused(name, args, o):
        with pytest.raises(RuntimeError, match=name):
            _call(name, cuda, *args)
        torch.cuda.synchronize()
        for k, t in o.items():
            assert bool((t == (9 if k == "arg" else mark)).all()), (name, k)
        assert float(rm.abs().max()) == 0.0 and bool((rv == 1).all())

    for k in (1, 2, 3, 6, 12, 24, 64):                   # s * k = 96 elements per row of the plane in every call
        s = 96 // k if 96 % k == 0 else 1
        o = outs()
        refused("batchnorm_train_relu_maxk_forward", (2, c, s, k, P(x), 0, 0, T.EPS, 0.1, P(rm), P(rv), P(o["pooled"]), P(o["arg"]),
                                                      P(o["xsel"]), P(o["sm"]), P(o["si"]), P(ws)), o)
        refused("batchnorm_train_relu_maxk_forward_devmom", (2, c, s, k, P(x), 0, 0, T.EPS, P(mom), P(rm), P(rv), P(o["pooled"]),
                                                             P(o["arg"]), P(o["xsel"]), P(o["sm"]), P(o["si"]), P(ws)), o)
        refused("batchnorm_train_relu_maxk_apply", (2, c, s, k, P(x), 0, 0, P(rm), P(rv), P(o["pooled"]), P(o["arg"]), P(o["xsel"])), o)
        arg0 = torch.zeros((2, 3, 96), dtype=torch.uint8, device=cuda)
        refused("batchnorm_train_relu_maxk_backward", (2, c, s, k, P(x), P(o["pooled"]), P(arg0), P(o["xsel"]), 0, 0, P(rm), P(rv),
                                                       P(o["dx"]), P(o["dg"]), P(o["db"]), P(ws)), o)
    for a, b_ in ((P(rm), 0), (0, P(rv))):               # exactly one of the running statistics
        o = outs()
        refused("batchnorm_train_forward", (2, c, 96, P(x), 0, 0, T.EPS, 0.1, a, b_, P(o["y"]), P(o["sm"]), P(o["si"]), P(ws), 0), o)
        refused("batchnorm_train_forward_devmom", (2, c, 96, P(x), 0, 0, T.EPS, P(mom), a, b_, P(o["y"]), P(o["sm"]), P(o["si"]),
                                                   P(ws), 0), o)
        refused("batchnorm_train_relu_maxk_forward", (2, c, 8, 8, P(x), 0, 0, T.EPS, 0.1, a, b_, P(o["pooled"]), P(o["arg"]),
                                                      P(o["xsel"]), P(o["sm"]), P(o["si"]), P(ws)), o)
    o = outs()                                           # running statistics and no momentum cell
    refused("batchnorm_train_forward_devmom", (2, c, 96, P(x), 0, 0, T.EPS, 0, P(rm), P(rv), P(o["y"]), P(o["sm"]), P(o["si"]),
                                               P(ws), 0), o)
    refused("batchnorm_train_relu_maxk_forward_devmom", (2, c, 8, 8, P(x), 0, 0, T.EPS, 0, P(rm), P(rv), P(o["pooled"]),
                                                         P(o["arg"]), P(o["xsel"]), P(o["sm"]), P(o["si"]), P(ws)), o)


@pytest.mark.parametrize("K", T.SOFTMAX_K)
def test_softmax_weighted_sum_every_k_against_float64(cuda, K):
    """softmax_wsum_fwd_kernel<K> / softmax_wsum_bwd_kernel<K> (K = 1, 6: scalar and float2 loads; the others float4) on 1, 255,
    256 and 257 rows: Gaussian logits, equal logits (power-of-two K: the mean of the integer values, bit for bit) and logits
    spread until expf underflows, within the row-wise bounds of bn_cases.softmax_reference."""
    from pwclonet_pylidarslam_amd import softmax_wsum as sw
    for rows in T.SOFTMAX_ROWS:
        for kind in T.SOFTMAX_KINDS:
            x, v, go = T.softmax_input(K, rows, kind)
            xd, vd = x.to(cuda).requires_grad_(True), v.to(cuda).requires_grad_(True)
            assert sw.supported(xd, vd)
            out = sw.softmax_weighted_sum(xd, vd)
            out.backward(go.to(cuda))
            (w_out, w_dx, w_dv), (b_out, b_dx, b_dv) = T.softmax_reference(x, v, go)
            _within("softmax.%s.out" % kind, out.detach(), w_out, b_out)
            _within("softmax.%s.dx" % kind, xd.grad, w_dx, b_dx)
            _within("softmax.%s.dv" % kind, vd.grad, w_dv, b_dv)
            if kind == "equal" and K & (K - 1) == 0:
                assert torch.equal(out.detach().cpu().double(), v.double().mean(3))
                assert torch.equal(vd.grad.cpu().double(), (go.double() / K).unsqueeze(3).expand(1, 1, rows, K))
