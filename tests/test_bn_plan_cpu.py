"""What csrc/batchnorm.hip launches for a shape, on the host, and what tests/test_gpu_bn_variants.py rests on:
batchnorm_train_plan_query (the launchers' own bn_splits(), host only) swept over a grid of (c, M, L) with the invariants
the kernels rely on, against the case tables of tests/bn_cases.py (every reachable form is reached); the exact boundary /
tie cases evaluated in numpy fp32, with and without fused multiply-add, equal their float64 evaluation bit for bit; on the
real-valued cases an fp32 evaluation of each kernel expression stays inside the bound the GPU test applies (the bounds are
not vacuous), the share of ReLU decisions within rounding of zero is below 1e-4, and the large-mean bound is sharp: an
fp32 one-pass variance misses it by more than 100 x.
"""
import numpy as np
import pytest
import torch

import bn_cases as T

C_GRID = (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 128, 512, 2048, 4096)
L_GRID = (1, 3, 4, 5, 12, 13, 16, 17, 255, 256, 257, 1020, 1023, 1024, 1025, 1028, 2051, 2052, 4096, 4097, 4100, 8192, 10003,
          10004, 133335, 133336, 524291, 524292)
B_GRID = (1, 2, 3, 9, 130, 511, 512, 803, 2500, 20300, 61500, 65300, 65535)


@pytest.fixture(scope="module")
def B():
    from pwclonet_pylidarslam_amd import batchnorm
    return batchnorm


@pytest.fixture(scope="module")
def reachable(B):
    """Forms the sweep selects, dense and max-K; the invariants of every plan on the way."""
    from pwclonet_pylidarslam_amd import _lib
    ws = {c: _lib.load().batchnorm_train_workspace_bytes(c) for c in C_GRID}
    dense = set()
    for c in C_GRID:
        for L in L_GRID:
            for b in B_GRID:
                M = b * L
                p = B.plan(c, M, L)
                n, ps = p["nsplit"], p["per_split"]
                assert ps % 4 == 0 and ps >= 4096, (c, M, L, p)          # a float4 never straddles a range; >= 4 per thread
                assert n * ps >= M > (n - 1) * ps and 1 <= n <= 256, (c, M, L, p)
                assert c * n * 16 <= ws[c], (c, M, L, p)
                assert p["vec"] == int(L % 4 == 0)
                dense.add(T.dense_form(p, c, L))
    maxk = set()
    for K in (4, 8, 16, 32):
        for c in (1, 2, 3, 5, 64):
            for b in (1, 2, 3, 5):
                for S in (1, 2, 3, 4, 5, 36, 37, 63, 64, 65, 128, 255, 256, 257, 1024, 2051, 2052, 2304, 4097, 5000):
                    maxk.add(T.maxk_form(B.plan(c, b * S, S), S, K))
                    assert B.plan(c, b * S * K, S * K)["vec"] == 1       # the forward's statistics pass: always 16-byte loads
    return dense, maxk


def test_plan_query_python_wrapper_and_arguments(B):
    assert B.plan(1, 4096, 4) == dict(nsplit=1, per_split=4096, vec=1)
    assert B.plan(1, 4097, 4097) == dict(nsplit=2, per_split=4096, vec=0)
    assert B.plan(8, 2 * 524292, 524292) == dict(nsplit=256, per_split=4100, vec=1)
    assert B.plan(9, 2 * 524292, 524292) == dict(nsplit=227, per_split=4620, vec=1)       # 2048 / 9 = 227 splits wanted
    assert B.plan(2048, 1 << 30, 5) == dict(nsplit=1, per_split=1 << 30, vec=0)
    assert B.plan(3, (1 << 40) + 1, 1)["nsplit"] == 256                                  # M beyond 32 bits
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 4, 4)):
        with pytest.raises(ValueError):
            B.plan(*bad)


def test_gpu_case_table_reaches_every_reachable_form(B, reachable):
    dense, maxk = reachable
    got = set()
    for c in T.DENSE_CASES:
        p = B.plan(c.c, c.b * c.L, c.L)
        assert T.dense_form(p, c.c, c.L) == c.want, (T.dense_id(c), p)
        got.add(c.want)
        assert c.b <= 65535 and c.b * c.c * c.L * 4 <= 8.5e6, T.dense_id(c)             # about 8 MB per tensor at the most
        if c.opts.get("short_last") and p["nsplit"] > 1:
            assert 0 < c.b * c.L - (p["nsplit"] - 1) * p["per_split"] < p["per_split"], (T.dense_id(c), p)
        if c.want[2] == "long":                 # every range begins and ends inside a row
            assert c.L > p["per_split"] and p["per_split"] % c.L != 0
    assert T.EXEMPT <= dense                    # the left-out forms exist, and only for want of memory:
    assert 3 * (255 * 4096 + 1) * 4 > 12e6      # the cap needs M > 255 * 4096, c % 4 in {3, 0} needs c >= 3
    assert got == dense - T.EXEMPT, ("not reached", sorted(dense - T.EXEMPT - got), "not reachable", sorted(got - dense))
    multi = [c for c in T.DENSE_CASES if c.want[1] != "1"]
    assert {(c.want[0], c.c % 4) for c in multi} == {(v, r) for v in (0, 1) for r in range(4)}
    assert any(c.c > 4 and c.c % 4 for c in multi)                  # a full finish workgroup and a partial one
    assert any(not c.opts.get("short_last") for c in multi)         # ... and equal splits
    # the shapes the issue names: L = 4 vec, L = 1 and L = 5 scalar with several loop iterations (M > one step of the 256 threads)
    for L, step in ((4, 1024), (1, 256), (5, 256)):
        assert any(c.L == L and c.b * c.L > 3 * step for c in T.DENSE_CASES)
    got_k = set()
    for m in T.MAXK_CASES:
        assert T.maxk_form(B.plan(m.c, m.b * m.S, m.S), m.S, m.K) == m.want, T.maxk_id(m)
        got_k.add(m.want)
    assert got_k == maxk, ("not reached", sorted(maxk - got_k), "not reachable", sorted(got_k - maxk))
    assert {m.S for m in T.MAXK_CASES} >= {1, 2051, 2052} and {m.K for m in T.MAXK_CASES} == {4, 8, 16, 32}
    print("\nbatchnorm forms reachable: dense %d (%d left out: > 8 MB), max-K %d" % (len(dense), len(T.EXEMPT), len(maxk)))


def _bits_equal(a32, b64):
    return a32.dtype == np.float32 and np.array_equal(a32.astype(np.float64), np.asarray(b64, dtype=np.float64))


@pytest.mark.parametrize("K", [4, 8, 16, 32])
def test_exact_cases_are_exact_in_fp32_with_and_without_fma(K):
    """Forward set (S = 1024: every position, every pair) and backward set (M = b S K = 2^13): every intermediate of
    yv = ((x - 0) * 1) * g + be and of dx = ((gv - c0) - xh * c1) * (g * 1) evaluated in fp32 -- separately rounded and with
    the product fused into the sum -- is the float64 value; the sums are integers (multiples of 1/8) below 2^24."""
    for b, S in ((2, 1024), (2, 4096 // K)):
        x, g, be, kinds, where = T.exact_maxk(K, b, S)
        if S == 1024:                                # every position, every pair (K = 32: 8 + 32 + 496 rows) and random rows
            assert set(kinds.tolist()) == set(range(7)) and int((kinds == T.KIND_TIE).sum()) == K * (K - 1) // 2
        C = x.shape[1]
        zero, one = torch.zeros(C), torch.ones(C)
        y64, _, xh64 = T.forward_reference(x, zero, one, g, be)
        assert torch.equal(xh64, x.double())
        gb, bb = g.numpy().reshape(1, C, 1, 1), be.numpy().reshape(1, C, 1, 1)
        for fma in (False, True):
            yv, xh = T.emulate_y(x.numpy(), 0.0, 1.0, gb, bb, fma)
            assert _bits_equal(yv, y64.numpy()) and _bits_equal(xh, x.numpy())
        pooled, arg, xsel = T.maxk_reference(x.double(), y64)
        # the constructions are what they say
        kd = torch.from_numpy(kinds)
        live = g != 0
        assert bool((arg[:, live][:, :, kd == T.KIND_UNIQUE] == torch.from_numpy(where[kinds == T.KIND_UNIQUE, 0]).to(torch.uint8)).all())
        assert bool((arg[:, live][:, :, kd == T.KIND_TIE] == torch.from_numpy(where[kinds == T.KIND_TIE, 0]).to(torch.uint8)).all())
        for k_, val in ((T.KIND_ZERO, 0.0), (T.KIND_MINUS, 0.0), (T.KIND_NONPOS, 0.0)):
            assert bool((pooled[:, live][:, :, kd == k_] == val).all())
        assert bool((pooled[:, ~live] == be[~live].double().clamp_min(0).reshape(1, -1, 1)).all())   # gamma = 0: relu(beta)
        assert bool((pooled[:, live][:, :, kd == T.KIND_PLUS] == (g[live].abs().double() / 8).reshape(1, -1, 1)).all())
        assert bool((arg[:, ~live] == 0).all()) and bool((arg[pooled == 0] == 0).all())
        neg = g < 0                                  # negative gamma: the maximum comes from the smallest x
        assert bool((xsel[:, neg][pooled[:, neg] > 0] == x.double()[:, neg].min(dim=3)[0][pooled[:, neg] > 0]).all())
        if b * S * K != 2 ** 13:
            continue
        M = b * S * K
        dpool = T.exact_dpool(b, C, S, K)
        dy = T.scatter_dpool(dpool.double(), arg, pooled, K)
        dgamma, dbeta, _, _ = T.sums_reference(xh64.reshape(b, C, -1), dy.reshape(b, C, -1))
        assert torch.equal(dbeta, (dpool.double() * (pooled > 0)).sum(dim=(0, 2))) and torch.equal(dbeta, dbeta.round())
        assert float(dy.abs().sum()) < 2 ** 24 / 64 and torch.equal(dgamma * 8, (dgamma * 8).round())
        assert torch.equal(dgamma.float().double(), dgamma) and torch.equal(dbeta.float().double(), dbeta)
        c0, c1 = T.kernel_c01(dgamma.float(), dbeta.float(), M)
        assert torch.equal(c0.double(), dbeta / M) and torch.equal(c1.double(), dgamma / M)
        dx64, _ = T.backward_reference(xh64, dy, one, g, c0, c1)
        for fma in (False, True):
            dx = T.emulate_dx(x.numpy(), dy.numpy(), c0.numpy().reshape(1, C, 1, 1), c1.numpy().reshape(1, C, 1, 1), gb, 1.0, fma)
            assert _bits_equal(dx, dx64.numpy()), (K, fma)


def _dense_check(case, family, relu, affine):
    x = T.dense_input(case, family)
    ref = T.stats_reference(x)
    bm, bv, bi = T.stats_bounds(ref)
    M = ref["M"]
    # the kernel's statistics expression, fp64 one-pass: inside the bounds
    x64 = x.double().transpose(0, 1).reshape(case.c, -1)
    mean = x64.sum(1) / M
    var = ((x64 * x64).sum(1) / M - mean * mean).clamp_min(0.0)
    assert bool(((mean.float().double() - ref["mean"]).abs() <= bm).all())
    assert bool(((var - ref["var"]).abs() <= bv).all())
    invstd = (1.0 / torch.sqrt(var + T.EPS)).float()
    assert bool(((invstd.double() - ref["invstd"]).abs() <= bi).all())
    if family == "const":
        assert float(ref["var"][0]) == 0.0 and float(bv[0]) < 1e-8
    return x, ref, mean.float(), invstd, bv


@pytest.mark.parametrize("case", T.DENSE_CASES, ids=T.dense_id)
def test_dense_bounds_hold_for_an_fp32_evaluation_and_the_large_mean_bound_is_sharp(case):
    for family in T.FAMILIES:
        x, ref, mean, invstd, bv = _dense_check(case, family, 1, 1)
        if family == "offset":
            # fp32 one-pass E[x^2] - mean^2 (numpy's pairwise fp32 sums): off by more than 100 bounds
            xc = x.numpy().transpose(1, 0, 2).reshape(case.c, -1)
            m32 = xc.sum(axis=1, dtype=np.float32) / np.float32(ref["M"])
            v32 = (xc * xc).sum(axis=1, dtype=np.float32) / np.float32(ref["M"]) - m32 * m32
            ratio = np.abs(v32.astype(np.float64) - ref["var"].numpy()) / bv.numpy()
            assert ratio.min() >= 100.0, ratio
            assert abs(float(ref["mean"][0]) - 6144) < 0.15 and abs(float(ref["var"][0]) - 2.25) < 0.45
            continue
        if family != "gauss":
            continue
        g, be = T.affine_params(case.c, 1)
        y64, by, xh = T.forward_reference(x, mean, invstd, g, be)
        amb = y64.abs() <= by
        assert float(amb.double().mean()) <= 1e-4
        sh = (1, case.c, 1)
        for fma in (False, True):
            yv, xh32 = T.emulate_y(x.numpy(), mean.numpy().reshape(sh), invstd.numpy().reshape(sh), g.numpy().reshape(sh),
                                   be.numpy().reshape(sh), fma)
            assert bool(((torch.from_numpy(yv).double() - y64).abs() <= by).all())
        dy = T.dense_grad(case).double()
        for relu in (0, 1):
            gv = dy * (y64 > 0) if relu else dy
            dgamma, dbeta, bg, bb = T.sums_reference(xh, gv, dy.abs() * amb if relu else None)
            # the reduction's expression: fp64 sums of gv * fp32 xhat
            gk = dy * torch.from_numpy(yv > 0) if relu else dy
            red = lambda t: t.transpose(0, 1).reshape(case.c, -1).sum(1)
            assert bool(((red(gk).float().double() - dbeta).abs() <= bb).all())
            assert bool(((red(gk * torch.from_numpy(xh32).double()).float().double() - dgamma).abs() <= bg).all())
            c0, c1 = T.kernel_c01(dgamma.float(), dbeta.float(), ref["M"])
            dx64, bdx = T.backward_reference(xh, gv, invstd, g, c0, c1)
            for fma in (False, True):
                dx = T.emulate_dx(xh32, gk.float().numpy(), c0.numpy().reshape(sh), c1.numpy().reshape(sh), g.numpy().reshape(sh),
                                  invstd.numpy().reshape(sh), fma)
                err = (torch.from_numpy(dx).double() - dx64).abs()
                assert bool(((err <= bdx) | amb).all()), float((err / bdx)[~amb].max())


@pytest.mark.parametrize("case", T.MAXK_CASES, ids=T.maxk_id)
def test_maxk_inputs_tie_and_stay_off_the_relu_boundary(case):
    x, dpool = T.maxk_input(case)
    ref = T.stats_reference(x.reshape(case.b, case.c, -1))
    g, be = T.affine_params(case.c, 1)
    y64, by, _ = T.forward_reference(x, ref["mean"].float(), ref["invstd"].float(), g, be)
    assert float((y64.abs() <= by).double().mean()) <= 1e-4
    if case.K * case.S >= 64:
        assert bool((x[..., 1:] == x[..., :1]).any())            # duplicated neighbours: exact ties inside rows


@pytest.mark.parametrize("K", T.SOFTMAX_K)
def test_softmax_bounds_hold_for_an_fp32_evaluation(K):
    for rows in T.SOFTMAX_ROWS:
        for kind in T.SOFTMAX_KINDS:
            x, v, go = T.softmax_input(K, rows, kind)
            (out, dx, dv), (b_out, b_dx, b_dv) = T.softmax_reference(x, v, go)
            e_out, e_dx, e_dv = T.emulate_softmax(x, v, go)
            for got, want, bound, what in ((e_out, out, b_out, "out"), (e_dx, dx, b_dx, "dx"), (e_dv, dv, b_dv, "dv")):
                err = (torch.from_numpy(got).double() - want[0, 0]).abs()
                assert bool((err <= bound[0, 0]).all()), (K, rows, kind, what, float((err / bound[0, 0]).max()))
            if kind == "equal" and K & (K - 1) == 0:              # p = 1 / K exactly: the mean of the integers
                assert np.array_equal(e_out.astype(np.float64), v.double().mean(3)[0, 0].numpy())
            if kind == "underflow" and K >= 4:
                assert bool((np.exp((x - x.max(3, keepdim=True)[0]).numpy()) == 0).any())
