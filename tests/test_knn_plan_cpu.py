"""What csrc/knn.hip launches for a shape, on the host: knn_point_plan_query (the launchers' own knn_plan()) against an
independent restatement of the thresholds over a sweep of (b, n, s, k); every one of the 19 instantiations the source
dispatches is selectable by a shape the entry points accept and reached by the case table of tests/knn_cases.py; K <= 32
with the rows switch on never falls through to the pruned kernel; the workspace layout agrees with the plan's block count;
and the table's clouds and queries are what their names say.
"""
import os
import re

import pytest
import torch

import knn_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B = (1, 2, 3, 32, 64)
N = (1, 5, 63, 64, 65, 255, 256, 257, 600, 1023, 1024, 1025, 1728, 1792, 1793, 2048, 2049, 2752, 2816, 2817, 3776, 3840, 3841, 4032,
     4033, 4096, 4097, 4544, 4608, 4609, 5568, 5632, 5633, 8192, 8193, 8640, 8704, 8705, 9664, 9728, 9729, 16320, 16321, 16384, 16385,
     20000)
S = (1, 5, 67, 255, 256, 300, 1024, 1025, 2048, 4096, 4097, 32768, 32769, 70000)
K = (1, 2, 15, 16, 17, 31, 32, 33, 48, 64)


@pytest.fixture(scope="module")
def E():
    from pwclonet_pylidarslam_amd.pointnet2_ops import _ext
    return _ext


def expected(b, n, s, k, prebuilt, use_rows, min_n=256, min_s=256):
    """The thresholds restated from the documentation of include/pwclo_ops.h, not from the launcher's code."""
    if not prebuilt and not (min_n <= n <= 16384 and s >= min_s):
        q = b * s
        qpw = 2 if q < 8192 else (4 if q < 65536 else 8)
        return dict(kernel="exhaustive", qpw=qpw, L=0, R=0, build_r=0, nslab=0, nblk=0, grid_x=-(-s // (4 * qpw)))
    data_blocks = -(-n // 64)
    nslab = 2 if data_blocks < 16 else (4 if data_blocks < 64 else (8 if data_blocks < 256 else 16))      # ~ sqrt(blocks) / 2
    nblk = data_blocks + nslab
    build_r = next(r for r in (1, 2, 4, 8, 16) if 1024 * r >= n)
    plan = dict(kernel="pruned", qpw=0, L=0, R=0, build_r=build_r, nslab=nslab, nblk=nblk, grid_x=-(-s // 4))
    if use_rows and k <= 32:
        L = 16 if k <= 16 else 32
        fit = [r for r in ((2, 3, 5, 9, 17) if L == 16 else (1, 2, 3, 5, 9)) if L * r >= nblk]
        if fit:
            plan.update(kernel="rows", L=L, R=min(fit), grid_x=-(-s // (4 * (64 // L))))
    return plan


def test_slab_rule_restated():
    """2 slabs below 16 blocks of points (961 points), 4 below 64 (4033), 8 below 256 (16321), 16 from there."""
    for n, want in ((64, 2), (960, 2), (961, 4), (4032, 4), (4033, 8), (16320, 8), (16321, 16), (16384, 16)):
        assert expected(1, n, 1, 1, True, True)["nslab"] == want, n


def test_plan_query_equals_the_restated_thresholds(E):
    min_n, min_s = int(os.environ.get("PWCLO_KNN_MIN_N", "256")), int(os.environ.get("PWCLO_KNN_MIN_S", "256"))
    checked = 0
    for n in N:
        for k in K:
            for b in B:
                for s in S:
                    for prebuilt in (False, True):
                        for rows in (False, True):
                            bad = k > n or (prebuilt and not 64 <= n <= 16384)
                            if bad:
                                with pytest.raises(ValueError):
                                    E.knn_point_plan(b, n, s, k, prebuilt=prebuilt, use_rows=rows)
                                continue
                            got = E.knn_point_plan(b, n, s, k, prebuilt=prebuilt, use_rows=rows)
                            assert got == expected(b, n, s, k, prebuilt, rows, min_n, min_s), (b, n, s, k, prebuilt, rows, got)
                            checked += 1
    assert checked > 50000


def test_plan_query_python_wrapper_and_arguments(E):
    assert E.knn_point_plan(2, 8192, 2048, 32, use_rows=True) == dict(kernel="rows", qpw=0, L=32, R=5, build_r=8, nslab=8, nblk=136,
                                                                      grid_x=256)
    assert E.knn_point_plan(2, 8192, 2048, 33) == dict(kernel="pruned", qpw=0, L=0, R=0, build_r=8, nslab=8, nblk=136, grid_x=512)
    assert E.knn_point_plan(32, 8192, 2048, 16, use_rows=False)["kernel"] == "pruned"
    assert E.knn_point_plan(2, 100, 2048, 16) == dict(kernel="exhaustive", qpw=2, L=0, R=0, build_r=0, nslab=0, nblk=0, grid_x=256)
    assert E.knn_point_plan(2, 100, 2048, 16, prebuilt=True, use_rows=True)["kernel"] == "rows"
    # use_rows=None: the switch as the launchers read it (PWCLO_KNN_ROWS, on unless set to 0)
    want = "rows" if int(os.environ.get("PWCLO_KNN_ROWS", "1")) else "pruned"
    assert E.knn_point_plan(2, 8192, 2048, 32)["kernel"] == want
    for bad in ((0, 100, 10, 4), (1, 0, 10, 4), (1, 100, 0, 4), (1, 100, 10, 0), (1, 100, 10, 65), (1, 10, 10, 11)):
        with pytest.raises(ValueError):
            E.knn_point_plan(*bad)
    for n in (63, 16385):
        with pytest.raises(ValueError):
            E.knn_point_plan(1, n, 10, 4, prebuilt=True)


def test_every_dispatched_instantiation_is_selectable_and_in_the_table(E):
    """The instantiations named in the source's dispatch == those the plan query can select over every n the entry points
    accept == those the case table reaches: 19."""
    src = open(os.path.join(ROOT, "pwclonet_pylidarslam_amd", "csrc", "knn.hip")).read()
    in_source = set("knn_kernel<%s>" % q for q in re.findall(r"hipLaunchKernelGGL\(knn_kernel<(\d+)>", src))
    in_source |= set("knn_build_kernel<%s>" % r for r in re.findall(r"KB_CASE\((\d+)\)", src))
    in_source |= set("knn_rows_kernel<%s,%s>" % lr for lr in re.findall(r"KR_CASE\((\d+), (\d+)\)", src))
    assert "hipLaunchKernelGGL(knn_pruned_kernel" in src
    in_source.add("knn_pruned_kernel")
    assert in_source == set(T.ALL_INSTANTIATIONS) and len(in_source) == 19
    # no kernel template of the file is launched from anywhere else
    assert set(re.findall(r"void (knn_\w*kernel)\(", src)) == {"knn_kernel", "knn_build_kernel", "knn_pruned_kernel", "knn_rows_kernel"}
    can = T.selectable()
    assert can == in_source, (sorted(in_source - can), sorted(can - in_source))
    reached = {}
    for case in T.CASES:
        plan = T.plan_of(case, use_rows=True)
        assert T.instantiations(plan) == case.want, (case.name, T.resolve_n(case), plan)
        for inst in case.want:
            reached.setdefault(inst, []).append(case.name)
    for case in T.ROWS0_CASES:
        assert T.instantiations(T.plan_of(case, use_rows=False)) == case.want and T.plan_of(case, use_rows=False)["kernel"] == "pruned"
        assert case.k <= 32 and T.plan_of(case, use_rows=True)["kernel"] == "rows"
        reached.setdefault("knn_pruned_kernel", []).append(case.name)
    assert set(reached) == can, sorted(can - set(reached))
    assert len({c.name for c in T.CASES}) == len(T.CASES)
    print()
    for inst in sorted(reached):
        print("%-26s %d cases: %s" % (inst, len(reached[inst]), " ".join(reached[inst][:6]) + (" ..." if len(reached[inst]) > 6 else "")))


def test_refiner_cases_select_their_kernels_and_were_missing(E):
    """The knn refiner's search forms at its smallest clouds: (b, n, s, k) = (12, 64, 64, 1), (3, 64, 64, 11), (3, 65, 65, 11),
    none of them a shape of the main table, each on the kernels it names; the model's knn agrees with the oracle on them."""
    import numpy as np

    import icp_model
    assert [(c.b, c.n, c.s, c.k) for c in T.REFINER_CASES] == [(12, 64, 64, 1), (3, 64, 64, 11), (3, 65, 65, 11)]
    have = {(c.b, c.n, c.s, c.k) for c in T.CASES if not isinstance(c.n, T.NBlk)}
    for case in T.REFINER_CASES:
        assert (case.b, case.n, case.s, case.k) not in have
        assert T.instantiations(T.plan_of(case, use_rows=True)) == case.want
        xyz, queries = T.refiner_inputs(case)
        assert xyz.shape == (case.b, case.n, 3) and queries.shape == (case.b, case.s, 3) and queries.dtype == torch.float32
        want = T.oracle(case, xyz, queries)
        for c in range(case.b):
            wi, wd = icp_model.knn(queries[c].numpy(), xyz[c].numpy(), case.k)
            assert np.array_equal(want[1][c].numpy(), wi) and np.array_equal(want[0][c].numpy().view(np.int32), wd.view(np.int32))
        if case.cloud == "lattice":                                  # ties at every rank: the index decides
            assert len(torch.unique(xyz[0], dim=0)) < case.n


def test_rows_bound_table_holds_every_block_of_every_n(E):
    """For every 64 <= n <= 16384, ceil(nblk / L) <= the largest R built for that L (17 for L = 16, 9 for L = 32): with the
    rows switch on, K <= 32 never falls through to the pruned kernel, and the R selected is the smallest that holds nblk."""
    most = 0
    for n in range(64, 16385):
        for k, L, rs in ((16, 16, (2, 3, 5, 9, 17)), (32, 32, (1, 2, 3, 5, 9))):
            plan = E.knn_point_plan(1, n, 300, k, prebuilt=True, use_rows=True)
            need = -(-plan["nblk"] // L)
            assert need <= rs[-1], (n, L, plan)
            assert plan["kernel"] == "rows" and plan["L"] == L and plan["R"] == min(r for r in rs if r >= need), (n, plan)
            most = max(most, plan["nblk"])
    assert most == T.MAX_BLOCKS and most <= 16 * 17 and most <= 32 * 9 and most <= 5 * 64     # KP_MAXR = 5 in the pruned kernel


def test_workspace_sections_agree_with_the_plan(E):
    import ctypes
    from pwclonet_pylidarslam_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_longlong * 4)()
    min_n = int(os.environ.get("PWCLO_KNN_MIN_N", "256"))
    for b in (1, 3):
        for n in (64, 255, 256, 257, 961, 4033, 8192, 16321, 16384):
            plan = E.knn_point_plan(b, n, 300, 8, prebuilt=True)
            assert lib.knn_point_slabs(n) == plan["nslab"]
            assert lib.knn_point_build_bytes(b, n) == b * plan["nblk"] * (64 * 16 + 32)
            ok = lib.knn_point_workspace_sections(b, n, out)
            if n < min_n:
                assert ok == 0 and list(out) == [0, 0, 0, 0] and lib.knn_point_workspace_bytes(b, n) == 0
                continue
            assert ok == 1 and list(out) == [0, plan["nblk"] * 64 * 16, b * plan["nblk"] * 64 * 16, plan["nblk"] * 32], (n, list(out))
            assert out[2] + b * out[3] == lib.knn_point_workspace_bytes(b, n) == lib.knn_point_build_bytes(b, n)
        assert lib.knn_point_workspace_bytes(b, 16385) == 0 and lib.knn_point_build_bytes(b, 16385) == 0


def test_table_holds_both_sides_of_every_boundary(E):
    ns = {c.name: T.resolve_n(c) for c in T.CASES}
    point = [c for c in T.CASES if c.entry == "point"]
    # rows kernels: the last n with t blocks and the first with t + 1, adjacent, selecting the two R; 272 blocks for either L
    for L, bounds in T.ROWS_BOUNDARIES.items():
        for t, r_lo, r_hi in bounds:
            lo, hi = ns["rows%d-nblk%d" % (L, t)], ns["rows%d-nblk%d" % (L, t + 1)]
            assert hi == lo + 1 and lo % 64 == 0
            k = L
            assert (E.knn_point_plan(1, lo, 300, k, use_rows=True)["R"], E.knn_point_plan(1, hi, 300, k, use_rows=True)["R"]) == (r_lo, r_hi)
    for want in ("knn_rows_kernel<16,17>", "knn_rows_kernel<32,9>"):
        assert any(T.plan_of(c)["nblk"] == T.MAX_BLOCKS for c in point if want in c.want), want
    # build kernels: n = 1024|1025 ... 8192|8193, 16384, and an n that is 1 mod 64
    sizes = {ns[c.name] for c in point if c.want[0].startswith("knn_build")}
    for t in T.BUILD_BOUNDARIES:
        assert {t, t + 1} <= sizes
        assert E.knn_point_plan(1, t, 300, 8)["build_r"] * 2 == E.knn_point_plan(1, t + 1, 300, 8)["build_r"]
    assert 16384 in sizes and any(n % 64 == 1 for n in sizes)
    # exhaustive: both sides of b * s = 8192 and 65536, s no multiple of 32
    q = sorted(c.b * c.s for c in T.CASES if c.want[0].startswith("knn_kernel"))
    assert any(8192 - 64 <= v < 8192 for v in q) and any(8192 <= v < 8192 + 64 for v in q)
    assert any(65536 - 64 <= v < 65536 for v in q) and any(65536 <= v < 65536 + 64 for v in q)
    assert all(c.s % 32 for c in T.CASES if c.want[0] in ("knn_kernel<4>", "knn_kernel<8>"))
    # pruned kernel: K = 33, 48, 64 at a small n, in the 2049..4096 band and at 16384; s no multiple of its 4 queries per workgroup
    pruned = [c for c in point if c.want[-1] == "knn_pruned_kernel"]
    for lo, hi in ((256, 1024), (2049, 4096), (16384, 16384)):
        assert {c.k for c in pruned if lo <= ns[c.name] <= hi} >= {33, 48, 64}, (lo, hi)
    assert all(c.s >= 256 for c in pruned) and any(c.s % 4 for c in pruned)
    assert {c.cloud for c in pruned} == set(T.CLOUD_KINDS)
    assert {c.cloud for c in point if "rows_kernel<16" in c.want[-1]} == set(T.CLOUD_KINDS)
    assert {c.cloud for c in point if "rows_kernel<32" in c.want[-1]} == set(T.CLOUD_KINDS)
    assert {c.query for c in T.CASES} == set(T.QUERY_KINDS)
    # prebuilt entry points below the thresholds: every (n, s) with K <= 16, 17..32 and > 32, and a slice of a wider structure
    pre = [c for c in T.CASES if c.entry == "prebuilt"]
    for n in (64, 65, 130, 255):
        for s in (1, 5, 67):
            ks = sorted(c.k for c in pre if (c.n, c.s) == (n, s))
            assert len(ks) == 3 and ks[0] <= 16 < ks[1] <= 32 < ks[2], (n, s, ks)
    assert any(c.entry == "slice" and c.n in (64, 65, 130, 255) for c in T.CASES)
    assert all(c.b <= 2 for c in T.CASES)


@pytest.mark.parametrize("kind", T.CLOUD_KINDS)
def test_cloud_kinds_are_what_they_say(kind):
    for n in (130, 600, 2500):
        x, y = T.make_cloud(kind, 1, n), T.make_cloud(kind, 1, n)
        assert x.shape == (n, 3) and x.dtype == torch.float32 and torch.equal(x, y) and bool(torch.isfinite(x).all())
        ext = x.max(0).values - x.min(0).values
        if kind == "same_x":
            assert ext[0] == 0 and ext[1] > 0 and ext[2] > 0
        elif kind == "same_z":
            assert ext[2] == 0 and ext[0] > 0
        elif kind == "identical":
            assert float(ext.max()) == 0
        elif kind == "line_y":
            assert ext[0] == 0 and ext[2] == 0 and ext[1] > 0
        elif kind == "lattice":
            assert len(torch.unique(x, dim=0)) < n and torch.equal(x, x.round())
        elif kind == "kitti_outlier":
            assert int((x[:, 0] == 1.0e6).sum()) == 1 and float(x[:, 0].kthvalue(n - 1).values) < 30
            # every other point lands in the first of the build's 1024 x-bins
            lo, hi = x[:, 0].min(), x[:, 0].max()
            bins = ((x[:, 0] - lo) * (1024.0 / (hi - lo))).int().clamp(0, 1023)
            assert int((bins == 0).sum()) == n - 1
        elif kind == "offset":
            assert float(x.abs().min()) > 4.9e3 and float(ext.max()) < 6.01
        elif kind == "clusters":
            centres = T.cluster_centres(n)
            for c in centres:
                c = c.clone()
                d = (x.double() - c.double()).norm(dim=1)
                members = torch.nonzero(d <= T.CLUSTER_RADIUS * 1.01).flatten()
                assert len(members) > 64, (n, len(members))
                # interleaved with the other clusters' members and the rest of the cloud: no two members adjacent when
                # there is more than one cluster
                assert len(centres) == 1 or int(members.diff().min()) >= 2
                t = ((x[members] - c) ** 2).sum(1)
                assert float(t.max()) < 1e-8
            # the first cluster is tighter than fp32 resolves at 1e-8: dozens of distinct squared distances, at most two keys
            t = ((x - centres[0]) ** 2).sum(1)
            t = t[t < 1e-13]
            assert len(t) > 64 and len(torch.unique(t)) > 16 and len(torch.unique(torch.sqrt(t + 1e-8))) <= 2


def test_query_kinds_are_what_they_say():
    x = T.make_cloud("clusters", 1, 2500)
    lo, hi = x.min(0).values, x.max(0).values
    ext = float((hi - lo).max())
    for kind in T.QUERY_KINDS:
        for s in (1, 5, 67, 301):
            q = T.make_queries(kind, 1, x, s)
            assert q.shape == (s, 3) and q.dtype == torch.float32 and bool(torch.isfinite(q).all())
    own = T.make_queries("own", 1, x, 301)
    assert bool((torch.cdist(own.double(), x.double()).min(1).values == 0).all())
    far = T.make_queries("far", 1, x, 301)
    assert float(torch.cdist(far.double(), x.double()).min()) > 90 * ext
    box = T.make_queries("box", 1, x, 301)
    on_face = ((box == lo) | (box == hi)).any(1)
    assert bool(on_face.all()) and bool(((box[:8] == lo) | (box[:8] == hi)).all())
    cen = T.make_queries("centres", 1, x, 301)
    assert torch.equal(cen[:4], T.cluster_centres(2500))
    # the far queries of the outlier cloud start along +x: nearest to the outlier, whose block holds one valid row
    xo = T.make_cloud("kitti_outlier", 1, 600)
    fo = T.make_queries("far", 1, xo, 601)
    assert int(torch.cdist(fo[:1].double(), xo.double()).argmin()) == int(xo[:, 0].argmax())
