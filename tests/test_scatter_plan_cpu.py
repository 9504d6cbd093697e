"""Which forms of the scatter-add gradient kernels (csrc/group_points.hip: gp_grad, csrc/interpolate.hip:
three_interpolate_grad) the host dispatch can select, and that tests/test_gpu_scatter_grads.py reaches all of them:
group_points_grad_plan_query / three_interpolate_grad_plan_query (the launchers' own gp_grad_plan() / ti_grad_plan(), host
only) swept over a grid of shapes, against the case table of tests/scatter_cases.py.  Also, on the CPU, the two properties
the GPU test rests on: the integer-valued inputs sum exactly in fp32 in any order, and on the real-valued inputs whose
error is compared with torch's fp32 index_add_, that reference's own error barely depends on the order.
"""
import pytest
import torch

import scatter_cases as T

B = (1, 2, 3, 4, 8, 16, 32, 63, 64, 128, 255, 256, 300)
C = (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 32, 33, 64, 65, 128)
N = (1, 3, 64, 1000) + tuple(t + d for t in T.THRESHOLDS for d in (0, 1)) + (100000,)
P = (1, 3, 4, 37, 148, 1024, 1025, 2048, 2049, 4096, 4100, 6148, 8193, 20000, 524288)


@pytest.fixture(scope="module")
def E():
    from pwclonet_pylidarslam_amd.pointnet2_ops import _ext
    return _ext


@pytest.fixture(scope="module")
def reachable(E):
    """-> (group forms, interpolate forms) that the sweep selects, with the LDS switch on and off, aligned and not."""
    grp, itp = set(), set()
    for b in B:
        for c in C:
            for n in N:
                for p in P:
                    for al in (0, 1):
                        plan = E.group_points_grad_plan(b, c, n, p, aligned=al, use_lds=True)
                        grp.add(T.group_form(plan, c))
                        # what the kernel relies on: 16-byte loads never straddle a range, the ranges cover P, the slices c
                        if plan["form"] == "lds":
                            assert plan["ct"] * n * 4 <= 128 * 1024 and 1 <= plan["ct"] <= 8, (b, c, n, p, plan)
                            assert plan["per_split"] % 4 == 0 and plan["ranges"] * plan["per_split"] >= p
                            assert (plan["ranges"] - 1) * plan["per_split"] < p and plan["ranges"] <= plan["splits"]
                            assert plan["slices"] * plan["ct"] >= c > (plan["slices"] - 1) * plan["ct"]
                            assert plan["vec4"] == int(p % 4 == 0 and al)
                            assert plan["ranges"] == 1 or plan["ct"] == 1
                        else:
                            assert n * 4 > 128 * 1024
                    assert T.group_form(E.group_points_grad_plan(b, c, n, p, use_lds=False), c) == ("atomic",)
                    plan = E.three_interpolate_grad_plan(b, c, p, n, use_lds=True)        # p fine points into n coarse ones
                    itp.add(T.interp_form(plan, c))
                    if plan["form"] == "lds":
                        assert plan["ct"] * n * 4 <= 128 * 1024 and 1 <= plan["ct"] <= 8
                        assert plan["ranges"] * plan["per_split"] >= p > (plan["ranges"] - 1) * plan["per_split"]
                        assert plan["slices"] * plan["ct"] >= c > (plan["slices"] - 1) * plan["ct"]
                        assert plan["vec4"] == 0 and (plan["ranges"] == 1 or plan["ct"] == 1)
                    assert T.interp_form(E.three_interpolate_grad_plan(b, c, p, n, use_lds=False), c) == ("atomic",)
    return grp, itp


def test_plan_query_python_wrapper_and_arguments(E):
    assert E.group_points_grad_plan(32, 64, 64, 148, use_lds=True) == dict(form="lds", ct=8, slices=8, splits=1, per_split=148,
                                                                           vec4=1, ranges=1)
    assert E.group_points_grad_plan(1, 3, 32768, 6148, use_lds=True) == dict(form="lds", ct=1, slices=3, splits=4,
                                                                             per_split=1540, vec4=1, ranges=4)
    assert E.group_points_grad_plan(1, 3, 32768, 6148, aligned=False, use_lds=True)["vec4"] == 0
    assert E.group_points_grad_plan(1, 3, 32769, 6148, use_lds=True)["form"] == "atomic"
    assert E.group_points_grad_plan(1, 3, 32768, 6148, use_lds=False)["form"] == "atomic"
    assert E.three_interpolate_grad_plan(1, 1, 4099, 64, use_lds=True) == dict(form="lds", ct=1, slices=1, splits=5,
                                                                               per_split=820, vec4=0, ranges=5)
    # use_lds=None: the switch as the launchers read it (PWCLO_GRAD_LDS, on unless set to 0)
    import os
    want = "lds" if int(os.environ.get("PWCLO_GRAD_LDS", "1")) else "atomic"
    assert E.group_points_grad_plan(2, 3, 64, 16)["form"] == want and E.three_interpolate_grad_plan(2, 3, 16, 64)["form"] == want
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)):
        with pytest.raises(ValueError):
            E.group_points_grad_plan(*bad)
        with pytest.raises(ValueError):
            E.three_interpolate_grad_plan(*bad)


def test_gpu_case_table_reaches_every_reachable_form(E, reachable):
    grp, itp = reachable
    got_g, got_i = set(), set()
    for c in T.GROUP_CASES:
        plan = E.group_points_grad_plan(c.b, c.c, c.n, c.s * c.k, aligned=True, use_lds=True)
        assert T.group_form(plan, c.c) == c.want, (T.case_id(c), plan)
        got_g.add(c.want)
        P_ = c.s * c.k
        assert plan["ranges"] == c.opts.get("ranges", plan["ranges"] if plan["form"] == "atomic" else 1), (T.case_id(c), plan)
        if c.opts.get("short"):          # a last range shorter than the others, and the boundaries inside the data
            assert 0 < P_ - (plan["ranges"] - 1) * plan["per_split"] < plan["per_split"], (T.case_id(c), plan)
    for c in T.INTERP_CASES:
        plan = E.three_interpolate_grad_plan(c.b, c.c, c.n, c.m, use_lds=True)
        assert T.interp_form(plan, c.c) == c.want, (T.case_id(c), plan)
        got_i.add(c.want)
        assert plan["ranges"] == c.opts.get("ranges", plan["ranges"] if plan["form"] == "atomic" else 1), (T.case_id(c), plan)
        if c.opts.get("short"):
            assert 0 < c.n - (plan["ranges"] - 1) * plan["per_split"] < plan["per_split"], (T.case_id(c), plan)
    # the misaligned scalar path is the aligned one's kernel code with vec4 = 0; torch hands out 16-byte aligned tensors,
    # so the table reaches vec4 = 0 through P % 4 != 0
    assert got_g == grp, ("not reached", sorted(grp - got_g), "not reachable", sorted(got_g - grp))
    assert got_i == itp, ("not reached", sorted(itp - got_i), "not reachable", sorted(got_i - itp))
    print("\nscatter-add forms reachable: group_points_grad %d, three_interpolate_grad %d" % (len(grp), len(itp)))
    # several ranges: P % 4 == 0 with equal ranges, P % 4 != 0, and a shorter last range
    multi = [c for c in T.GROUP_CASES if c.want[0] == "lds" and c.want[2]]
    assert any(c.want[3] == 1 and not c.opts.get("short") for c in multi)
    assert any(c.want[3] == 0 for c in multi) and any(c.want[3] == 1 and c.opts.get("short") for c in multi)
    for c in T.GATHER_CASES:             # gather_points_grad: group_points_grad with one sample per centre up to n = 32768
        if c.n * 4 <= 128 * 1024:
            assert T.group_form(E.group_points_grad_plan(c.b, c.c, c.n, c.m, use_lds=True), c.c) == c.want, T.case_id(c)
        else:
            assert c.want == ("gather",)
    assert {c.m for c in T.GATHER_CASES} >= {1} and {c.c for c in T.GATHER_CASES} >= {65}
    assert {c.want == ("gather",) for c in T.GATHER_CASES} == {False, True}
    assert {c.want == ("gather",) for c in T.GATHER_CASES if c.opts.get("perm")} == {False, True}     # m == n in both kernels


def test_case_table_holds_both_sides_of_every_size_threshold(E):
    for cases, size, plan_of in ((T.GROUP_CASES, lambda c: c.n, lambda c, n: E.group_points_grad_plan(c.b, c.c, n, c.s * c.k,
                                                                                                     use_lds=True)),
                                 (T.INTERP_CASES, lambda c: c.m, lambda c, m: E.three_interpolate_grad_plan(c.b, c.c, c.n, m,
                                                                                                            use_lds=True))):
        sizes = {size(c) for c in cases}
        for t in T.THRESHOLDS:
            assert {t, t + 1} <= sizes, t
            # and the threshold is live in the rows that sit on it: one more target changes ct, or the kernel
            below = [c for c in cases if size(c) == t]
            assert any((plan_of(c, t)["form"], plan_of(c, t)["ct"]) != (plan_of(c, t + 1)["form"], plan_of(c, t + 1)["ct"])
                       for c in below), t
        assert any(size(c) == 32768 and c.want[0] == "lds" for c in cases)
        assert any(size(c) == 32769 and c.want == ("atomic",) for c in cases)


ALL_CASES = T.GROUP_CASES + T.INTERP_CASES + T.GATHER_CASES


@pytest.mark.parametrize("case", ALL_CASES, ids=T.case_id)
def test_reference_is_exact_on_integer_inputs_and_order_blind_on_real_ones(case):
    """Integer-valued cases: every contribution is a multiple of q (1, or 0.25 with the fractional weights) and the sum of
    their magnitudes per target stays below 2^24 q, so every partial sum in every order is exact in fp32 -- shown for the
    reference itself in two orders.  Real-valued uniform / clustered cases: the fp32 index_add_ error that the GPU's RMS
    error is measured in is non-zero (or no target takes more than two contributions, and both orders are exact), and
    summing the positions in reverse changes it by far less than the margin of 4."""
    P_, n = T.positions(case)
    for dist in T.distributions(case):
        idx = T.make_idx(case, dist)
        assert idx.shape == (case.b, P_) and idx.dtype == torch.int32 and 0 <= int(idx.min()) and int(idx.max()) < n
        for kind in T.kinds(case):
            v, v64, _ = T.make_values(case, kind, dist)
            want, cnt, mag = T.exact(v64, idx, n)
            if dist == "permutation":
                assert int(cnt.min()) == 1 == int(cnt.max())
            fwd, rev = T.index_add32(v, idx, n), T.index_add32(v, idx, n, reverse=True)
            if kind != "real":
                q = 0.25 if kind == "int" and isinstance(case, T.Interp) else 1.0
                assert float(cnt.max()) * 16 < 2 ** 24 and float(mag.max()) / q < 2 ** 24
                assert torch.equal(v.double(), v64) and torch.equal(v64 / q, (v64 / q).round())
                assert torch.equal(fwd.double(), want) and torch.equal(rev.double(), want), (dist, kind)
                assert torch.equal(want.float().double(), want)
            elif dist == "permutation":
                assert torch.equal(fwd, want.float()) and torch.equal(v, v64.float())     # one contribution, rounded once
            else:
                bound = T.rounding_bound(cnt, mag)
                assert bool(((fwd.double() - want).abs() <= bound).all()) and bool(((rev.double() - want).abs() <= bound).all())
                if dist in ("uniform", "clustered"):
                    ef, er = T.rms(fwd.double() - want), T.rms(rev.double() - want)
                    if ef == 0.0:
                        assert int(cnt.max()) <= 2 and er == 0.0, (dist, float(cnt.max()))
                    else:
                        assert er / ef < T.RMS_MARGIN and ef / er < T.RMS_MARGIN, (dist, ef, er)
