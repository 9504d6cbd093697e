"""The case table of tests/test_gpu_knn_variants.py, with its clouds and queries, shared with tests/test_knn_plan_cpu.py, which
proves through knn_point_plan_query that the rows reach every kernel instantiation csrc/knn.hip can launch and sit on both
sides of every size threshold.

A case is (entry point, B, K, N, S, cloud kind, query kind) and the instantiations it is meant to launch:

  knn_kernel<2|4|8>                 exhaustive, by B * S (< 8192, < 65536, more); n < 256 or S < 256 through ``knn_point``
  knn_build_kernel<1|2|4|8|16>      the sort behind every other search: ceil(n / 1024) points per thread
  knn_rows_kernel<16,{2,3,5,9,17}>  K <= 16: R = block bounds per lane, the smallest with 16 R >= nblk = ceil(n / 64) + slabs
  knn_rows_kernel<32,{1,2,3,5,9}>   17 <= K <= 32, 32 R >= nblk
  knn_pruned_kernel                 K > 32, and every K in a process started with PWCLO_KNN_ROWS=0 (``--rows0`` below)

Entry points: "point" = ``_ext.knn_point`` (knn_point_ws_kernel_wrapper: 256 <= n <= 16384 and S >= 256 search a structure,
the rest is exhaustive); "prebuilt" = knn_build_kernel_wrapper + knn_point_prebuilt_kernel_wrapper, which take any
64 <= n <= 16384 and any S; "slice" = the same on clouds [1, 1 + B) of a structure built for B + 2 clouds.

N is a number, or ``NBlk(t, side)``: the first / last n whose structure has t blocks, found by scanning the plan query (the
register-count boundaries of the rows kernels are stated in blocks; the table cannot go stale when the slab rule moves).

There are two tables.  ``CASES`` is the one every sweep runs over (reachability, every instantiation, both sides of every
boundary).  ``REFINER_CASES`` holds the three search shapes of the knn refiner (registration.IcpRefiner) with their own
inputs (``refiner_inputs``) and their own truth (tests/icp_model.py's knn, and the oracle); the sweeps over ``CASES`` do not
see them, and they add no instantiation that ``CASES`` does not reach.

Everything here is CPU torch / numpy.  ``python tests/knn_cases.py --rows0`` is the child process of the PWCLO_KNN_ROWS=0
test: it checks K <= 32 on the pruned kernel against the oracle and exits non-zero on any difference.
"""
import functools
import os
import sys
from collections import namedtuple

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

Case = namedtuple("Case", "name entry b k n s cloud query want")
NBlk = namedtuple("NBlk", "blocks side")             # side: "first" / "last" n with that many blocks


def _ex(qpw):
    return ("knn_kernel<%d>" % qpw,)


def _rows(build, L, R):
    return ("knn_build_kernel<%d>" % build, "knn_rows_kernel<%d,%d>" % (L, R))


def _pruned(build):
    return ("knn_build_kernel<%d>" % build, "knn_pruned_kernel")


ALL_INSTANTIATIONS = frozenset(
    ["knn_kernel<%d>" % q for q in (2, 4, 8)] + ["knn_build_kernel<%d>" % r for r in (1, 2, 4, 8, 16)]
    + ["knn_rows_kernel<16,%d>" % r for r in (2, 3, 5, 9, 17)] + ["knn_rows_kernel<32,%d>" % r for r in (1, 2, 3, 5, 9)]
    + ["knn_pruned_kernel"])

CLOUD_KINDS = ("uniform", "lattice", "same_x", "same_z", "identical", "line_y", "kitti_outlier", "offset", "clusters")
QUERY_KINDS = ("own", "far", "box", "centres", "uniform")

# register-count boundaries of knn_rows_kernel<L, R> in blocks: the last nblk of one R | the first of the next
ROWS_BOUNDARIES = {16: ((32, 2, 3), (48, 3, 5), (80, 5, 9), (144, 9, 17)), 32: ((32, 1, 2), (64, 2, 3), (96, 3, 5), (160, 5, 9))}
MAX_BLOCKS = 272                                     # n in 16321..16384: 256 blocks of points + 16 slabs
BUILD_BOUNDARIES = (1024, 2048, 4096, 8192)          # the last n of knn_build_kernel<1|2|4|8>


def _build_of(blocks):
    """knn_build_kernel<R> of the boundary clouds (their n follows from the block count; test_knn_plan_cpu checks it)."""
    return {32: 2, 33: 2, 48: 4, 49: 4, 64: 4, 65: 4, 80: 8, 81: 8, 96: 8, 97: 8, 144: 16, 145: 16, 160: 16, 161: 16}[blocks]


def _boundary_cases():
    out = []
    geo = [("same_x", "own"), ("kitti_outlier", "far"), ("clusters", "centres"), ("lattice", "own"), ("offset", "uniform"),
           ("line_y", "box"), ("same_z", "far"), ("identical", "own"), ("uniform", "box"), ("kitti_outlier", "box")]
    i = 0
    for L, k in ((16, 16), (32, 32)):
        for t, r_lo, r_hi in ROWS_BOUNDARIES[L]:
            for blocks, side, r in ((t, "last", r_lo), (t + 1, "first", r_hi)):
                cloud, query = geo[i % len(geo)]
                i += 1
                out.append(Case("rows%d-nblk%d" % (L, blocks), "point", 1, k if i % 3 else k - 3, NBlk(blocks, side), 261 + 2 * i,
                                cloud, query, _rows(_build_of(blocks), L, r)))
    # the most blocks n <= 16384 allows: the largest bound table of either L must hold all of them
    out.append(Case("rows16-nblk272", "point", 1, 16, 16384, 263, "kitti_outlier", "own", _rows(16, 16, 17)))
    out.append(Case("rows32-nblk272", "point", 1, 32, 16384, 263, "clusters", "centres", _rows(16, 32, 9)))
    out.append(Case("rows16-nblk272-first", "point", 1, 9, NBlk(272, "first"), 259, "lattice", "box", _rows(16, 16, 17)))
    return out


def _build_cases():
    """n = 1024|1025, 2048|2049, 4096|4097, 8192|8193, 16384 and one n that is 1 mod 64, alternating K <= 16 and K <= 32."""
    rows = {1024: (1, 2, 1), 1025: (2, 2, 1), 2048: (2, 3, 2), 2049: (4, 3, 2), 2113: (4, 3, 2), 4096: (4, 5, 3), 4097: (8, 5, 3),
            8192: (8, 9, 5), 8193: (16, 9, 5), 16384: (16, 17, 9)}
    geo = [("uniform", "uniform"), ("lattice", "own"), ("same_z", "box"), ("offset", "own"), ("kitti_outlier", "uniform")]
    out = []
    for i, (n, (build, r16, r32)) in enumerate(sorted(rows.items())):
        cloud, query = geo[i % len(geo)]
        if i % 2 == 0:
            out.append(Case("build-n%d-k6" % n, "point", 2, 6, n, 301, cloud, query, _rows(build, 16, r16)))
        else:
            out.append(Case("build-n%d-k20" % n, "point", 2, 20, n, 301, cloud, query, _rows(build, 32, r32)))
    return out


def _pruned_cases():
    """K = 33, 48, 64 at n = 600 (K is more than half a block), in the 2049..4096 band and at 16384: one cloud kind each."""
    out = []
    kinds = iter(CLOUD_KINDS)
    queries = {"uniform": "uniform", "lattice": "own", "same_x": "box", "same_z": "own", "identical": "far", "line_y": "own",
               "kitti_outlier": "box", "offset": "far", "clusters": "centres"}
    for n, build, s, b in ((600, 1, 259, 2), (3000, 4, 301, 2), (16384, 16, 257, 1)):
        for k in (33, 48, 64):
            cloud = next(kinds)
            out.append(Case("pruned-n%d-k%d" % (n, k), "point", b, k, n, s, cloud, queries[cloud], _pruned(build)))
    # the nearest block of a query far out on +x is the outlier's slab: one valid row, so with K = 64 the bound stays infinite
    # over the following blocks; s = 601 is 1 mod the 4 queries of a workgroup
    out.append(Case("pruned-k64-sparse-first-block", "point", 2, 64, 600, 601, "kitti_outlier", "far", _pruned(1)))
    out.append(Case("pruned-k64-n256", "point", 2, 64, 256, 258, "clusters", "own", _pruned(1)))
    return out


def _geometry_cases():
    """Every cloud kind on a rows kernel of either L and on the pruned kernel, n = 2500 (4 slabs, 44 blocks)."""
    pairs = [("uniform", "uniform"), ("uniform", "box"), ("lattice", "own"), ("lattice", "far"), ("same_x", "own"), ("same_x", "box"),
             ("same_z", "far"), ("same_z", "uniform"), ("identical", "own"), ("identical", "far"), ("line_y", "box"),
             ("line_y", "far"), ("kitti_outlier", "far"), ("kitti_outlier", "box"), ("kitti_outlier", "own"), ("offset", "own"),
             ("offset", "uniform"), ("clusters", "centres"), ("clusters", "own")]
    out = []
    for cloud, query in pairs:
        for k, want in ((16, _rows(4, 16, 3)), (32, _rows(4, 32, 2)), (48, _pruned(4))):
            out.append(Case("geo-%s-%s-k%d" % (cloud, query, k), "point", 2, k, 2500, 300 + k % 5, cloud, query, want))
    return out


def _prebuilt_cases():
    """The prebuilt entry points below the product's thresholds: 3..6 blocks, mostly padding rows and empty boxes."""
    out = []
    kinds = [k for k in CLOUD_KINDS]
    i = 0
    for n in (64, 65, 130, 255):
        for s in (1, 5, 67):
            for k, want in ((11, _rows(1, 16, 2)), (32 if n % 2 else 19, _rows(1, 32, 1)), (64 if n != 130 else 41, _pruned(1))):
                cloud = kinds[i % len(kinds)]
                if cloud == "clusters" and n < 100:
                    cloud = "uniform"
                query = QUERY_KINDS[i % len(QUERY_KINDS)]
                if query == "centres" and cloud != "clusters":
                    query = "own"
                i += 1
                out.append(Case("prebuilt-n%d-s%d-k%d" % (n, s, k), "prebuilt", 2, k, n, s, cloud, query, want))
    out.append(Case("slice-n130-k16", "slice", 2, 16, 130, 67, "lattice", "own", _rows(1, 16, 2)))
    out.append(Case("slice-n255-k40", "slice", 2, 40, 255, 5, "uniform", "uniform", _pruned(1)))
    out.append(Case("slice-n2500-k32", "slice", 1, 32, 2500, 67, "kitti_outlier", "own", _rows(4, 32, 2)))
    return out


CASES = (
    [   # ---- exhaustive: both sides of B * S = 8192 and 65536 on a tiny cloud, S no multiple of 32; K = 64 = most of the cloud
        Case("ex2-small", "point", 2, 8, 70, 37, "uniform", "own", _ex(2)),
        Case("ex2-below-8192", "point", 2, 8, 70, 4095, "lattice", "uniform", _ex(2)),
        Case("ex4-above-8192", "point", 2, 8, 70, 4099, "lattice", "uniform", _ex(4)),
        Case("ex4-k64", "point", 1, 64, 70, 8195, "uniform", "uniform", _ex(4)),
        Case("ex4-below-65536", "point", 2, 8, 70, 32767, "uniform", "box", _ex(4)),
        Case("ex8-above-65536", "point", 2, 8, 70, 32771, "uniform", "box", _ex(8)),
        Case("ex8-k33-identical", "point", 2, 33, 66, 32769, "identical", "own", _ex(8)),
        # a cloud the structure would take, with too few queries to amortise the build
        Case("ex2-s255", "point", 2, 16, 2500, 255, "kitti_outlier", "own", _ex(2)),
    ]
    + _build_cases() + _boundary_cases() + _pruned_cases() + _geometry_cases() + _prebuilt_cases())

# the child process under PWCLO_KNN_ROWS=0: K <= 32 on knn_pruned_kernel, two cloud kinds
ROWS0_CASES = [Case("rows0-%s-k%d" % (cloud, k), "point", 2, k, 2500, 301, cloud, query, _pruned(4))
               for cloud, query in (("lattice", "own"), ("kitti_outlier", "box")) for k in (1, 6, 16, 32)]


# The search forms of the knn refiner (registration.IcpRefiner) at its smallest clouds: one iteration's search, K = 1 over
# S * M = 12 clouds of the frame's moved points, and the staging's own-neighbour lists, K = k_normals + 1 = 11 with every
# point of a cloud as a query.  No (b, n, s, k) of these was in CASES (its prebuilt rows have b = 2 and s = 1, 5, 67).  A table
# of its own: CASES keeps b <= 2, and these are compared with tests/icp_model.py's knn, the registration model's search.
REFINER_CASES = [Case("refiner-search-b12-n64-k1", "prebuilt", 12, 1, 64, 64, "uniform", "moved", _rows(1, 16, 2)),
                 Case("refiner-self-b3-n64-k11", "prebuilt", 3, 11, 64, 64, "lattice", "self", _rows(1, 16, 2)),
                 Case("refiner-self-b3-n65-k11", "prebuilt", 3, 11, 65, 65, "uniform", "self", _rows(1, 16, 2))]


def refiner_inputs(case):
    """-> xyz (b, n, 3), queries (b, n, 3): the clouds themselves ("self") or the clouds turned by 0.05 rad about z and
    shifted by a few centimetres ("moved"), rounded to fp32 once, as icp_queries_kernel hands them to the search."""
    xyz = torch.stack([make_cloud(case.cloud, 1 + i, case.n) for i in range(case.b)]).contiguous()
    if case.query == "self":
        return xyz, xyz.clone()
    c, s = np.cos(0.05), np.sin(0.05)
    rot = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    moved = xyz.double() @ rot.T + torch.tensor([0.07, -0.03, 0.02], dtype=torch.float64)
    return xyz, moved.float().contiguous()


def case_id(c):
    return c.name


# ---- what a plan answer launches -----------------------------------------------------------------------------------------
def instantiations(plan):
    """The kernel instantiations of a ``_ext.knn_point_plan`` answer, in launch order."""
    if plan["kernel"] == "exhaustive":
        return ("knn_kernel<%d>" % plan["qpw"],)
    search = "knn_rows_kernel<%d,%d>" % (plan["L"], plan["R"]) if plan["kernel"] == "rows" else "knn_pruned_kernel"
    return ("knn_build_kernel<%d>" % plan["build_r"], search)


@functools.lru_cache(maxsize=None)
def _blocks_table():
    """nblk of every 64 <= n <= 16384, through the plan query."""
    from pwclonet_pylidarslam_amd.pointnet2_ops import _ext
    return {n: _ext.knn_point_plan(1, n, 1, 1, prebuilt=True)["nblk"] for n in range(64, 16385)}


@functools.lru_cache(maxsize=None)
def selectable():
    """Every instantiation the plan query names for some shape the entry points accept: all n of the prebuilt entry points
    (no gate) at K on both sides of 16 | 17 and 32 | 33 with the rows switch on and off, and the exhaustive forms by B * S."""
    from pwclonet_pylidarslam_amd.pointnet2_ops import _ext
    out = set()
    for n in range(64, 16385):
        for k in (1, 16, 17, 32, 33, 64):
            for rows in (True, False):
                out.update(instantiations(_ext.knn_point_plan(1, n, 300, k, prebuilt=True, use_rows=rows)))
    for b, s in ((1, 1), (2, 4095), (2, 4096), (1, 65535), (1, 65536), (32, 2048), (64, 100000)):
        out.update(instantiations(_ext.knn_point_plan(b, 100, s, 8)))
    return frozenset(out)


def resolve_n(case):
    if not isinstance(case.n, NBlk):
        return case.n
    ns = [n for n, blocks in _blocks_table().items() if blocks == case.n.blocks and n >= 256]
    assert ns, "no n in [256, 16384] has %d blocks" % case.n.blocks
    return min(ns) if case.n.side == "first" else max(ns)


def plan_of(case, use_rows=None):
    from pwclonet_pylidarslam_amd.pointnet2_ops import _ext
    return _ext.knn_point_plan(case.b, resolve_n(case), case.s, case.k, prebuilt=case.entry != "point", use_rows=use_rows)


# ---- clouds: functions of (seed, n) -> (n, 3) fp32 ------------------------------------------------------------------------
CLUSTER_CENTRES = ((0.01, 0.02, -0.015), (5.0, -3.0, 1.0), (-12.0, 8.0, -2.0), (0.5, 0.25, -0.125))
CLUSTER_SIZE = 80                                     # > 64: a cluster's ties span more than one block of rows
CLUSTER_RADIUS = 3e-5                                 # t <= 3.6e-9 between members: below the 1e-8 under the square root
TIGHT_RADIUS = 3e-8                                   # the first cluster: t <= 3.6e-15 is below the spacing of fp32 at 1e-8, so
                                                      # distinct t share a key and the index alone orders the members


def cluster_centres(n):
    return torch.tensor(CLUSTER_CENTRES[:max(1, min(len(CLUSTER_CENTRES), n // 100))])


@functools.lru_cache(maxsize=None)
def _kitti(seed):
    from pwclonet_pylidarslam_amd import synthetic
    pc, _, _, _ = synthetic.kitti_like_pair(seed, 8192, 1)
    return torch.from_numpy(np.ascontiguousarray(pc[0, :, :3]))


def make_cloud(kind, seed, n):
    gen = torch.Generator().manual_seed(seed * 7919 + n * 31 + CLOUD_KINDS.index(kind))
    uni = (torch.rand(n, 3, generator=gen) * 2 - 1) * 20
    if kind == "uniform":
        return uni
    if kind == "lattice":                             # exact ties at every rank, duplicated points
        return torch.randint(-4, 5, (n, 3), generator=gen).float()
    if kind == "same_x":                              # zero extent in x: one x-bin, one slab
        uni[:, 0] = 3.25
        return uni
    if kind == "same_z":                              # zero extent in z: one z-bin per slab
        uni[:, 2] = -1.5
        return uni
    if kind == "identical":                           # every key equal: the index alone orders the list
        return torch.tensor([1.5, -2.25, 7.0]).repeat(n, 1)
    if kind == "line_y":
        uni[:, 0], uni[:, 2] = 2.0, -3.0
        return uni
    if kind == "kitti_outlier":                       # one point at x = 1e6: every other point falls into x-bin 0
        base = _kitti(90 + seed % 2)
        x = base.repeat((n + 8191) // 8192, 1)[:n].clone()        # n > 8192: exact duplicates
        x[(seed * 131 + n // 3) % n, 0] = 1.0e6
        return x
    if kind == "offset":                              # world coordinates: fp32 spacing 1e-3 at 1e4, exact ties between neighbours
        return (torch.rand(n, 3, generator=gen) * 2 - 1) * 3 + torch.tensor([1.0e4, -1.0e4, 5.0e3])
    assert kind == "clusters" and n >= 100
    centres = cluster_centres(n)
    ncl = len(centres)
    size = min(CLUSTER_SIZE, n // ncl - 1)
    step = max(1, n // (ncl * size))                  # member j of cluster c at index (j * ncl + c) * step: interleaved, spread
    for c in range(ncl):
        members = (torch.arange(size) * ncl + c) * step
        assert int(members.max()) < n
        off = (torch.rand(size, 3, generator=gen) * 2 - 1) * ((TIGHT_RADIUS if c == 0 else CLUSTER_RADIUS) / 3 ** 0.5)
        uni[members] = centres[c] + off
    return uni


def make_queries(kind, seed, cloud, s):
    """(s, 3) queries of one cloud (n, 3)."""
    n = cloud.shape[0]
    gen = torch.Generator().manual_seed(seed * 104729 + s * 17 + QUERY_KINDS.index(kind))
    lo, hi = cloud.min(0).values, cloud.max(0).values
    mid, ext = (lo + hi) / 2, float((hi - lo).max())
    pick = torch.randint(0, n, (s,), generator=gen)
    if kind == "own":                                 # t = 0 to the point itself (and to its duplicates)
        return cloud[pick].clone()
    if kind == "far":                                 # 100 x the extent away, along the axes first, then the diagonals
        dirs = torch.tensor([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 1], [-1, 1, -1],
                             [1, -1, 0], [0, 1, -1]], dtype=torch.float32)
        return mid + 100.0 * max(ext, 1.0) * dirs[torch.arange(s) % len(dirs)] + (cloud[pick] - mid)
    if kind == "box":                                 # the 8 corners and 6 face centres, then cloud points pushed onto a face
        pts = [torch.tensor([x, y, z]) for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]
        for ax in range(3):
            for v in (lo[ax], hi[ax]):
                p = mid.clone()
                p[ax] = v
                pts.append(p)
        q = cloud[pick].clone()
        ax = torch.arange(s) % 3
        q[torch.arange(s), ax] = torch.where(torch.arange(s) % 2 == 0, lo[ax], hi[ax])
        fixed = torch.stack(pts)[:s]
        q[:len(fixed)] = fixed
        return q
    if kind == "centres":                             # the exact centres, then points a few 1e-6 beside them
        centres = cluster_centres(n)
        q = centres[torch.arange(s) % len(centres)].clone()
        jitter = (torch.rand(s, 3, generator=gen) * 2 - 1) * 1e-5
        jitter[:len(centres)] = 0
        return q + jitter
    assert kind == "uniform"
    return mid + (torch.rand(s, 3, generator=gen) * 2 - 1) * (hi - lo + 1.0) * 0.6


def make_inputs(case, extra_clouds=0):
    """-> xyz (b + extra, n, 3), new_xyz (b + extra, s, 3), contiguous fp32 on the CPU; cloud i is seeded by i."""
    n = resolve_n(case)
    clouds = [make_cloud(case.cloud, 1 + i, n) for i in range(case.b + extra_clouds)]
    queries = [make_queries(case.query, 1 + i, c, case.s) for i, c in enumerate(clouds)]
    xyz, new_xyz = torch.stack(clouds).contiguous(), torch.stack(queries).contiguous()
    assert xyz.dtype == torch.float32 and new_xyz.dtype == torch.float32
    assert bool(torch.isfinite(xyz).all()) and bool(torch.isfinite(new_xyz).all())
    return xyz, new_xyz


# ---- running an entry point --------------------------------------------------------------------------------------------------
def run(case, xyz, new_xyz, dev, exhaustive=None):
    """-> (dist, idx) of the case's entry point on ``dev`` for CPU inputs (``make_inputs``; "slice": with_extra = 2)."""
    from pwclonet_pylidarslam_amd import _lib
    from pwclonet_pylidarslam_amd.pointnet2_ops import _ext
    k = case.k
    if case.entry == "point" or exhaustive:
        if case.entry == "slice":
            xyz, new_xyz = xyz[1:1 + case.b].contiguous(), new_xyz[1:1 + case.b].contiguous()
        return _ext.knn_point(k, xyz.to(dev), new_xyz.to(dev), return_dist=True, exhaustive=exhaustive)
    built_b, n, _ = xyz.shape
    x = xyz.to(dev)
    lib = _lib.load()
    ws = torch.empty((lib.knn_point_build_bytes(built_b, n),), dtype=torch.uint8, device=dev)
    _lib.call("knn_build_kernel_wrapper", dev, built_b, n, x.data_ptr(), ws.data_ptr(), 0)
    first = 1 if case.entry == "slice" else 0
    q = new_xyz[first:first + case.b].contiguous().to(dev)
    idx = torch.empty((case.b, case.s, k), dtype=torch.int32, device=dev)
    dist = torch.empty((case.b, case.s, k), dtype=torch.float32, device=dev)
    if case.entry == "slice":
        _lib.call("knn_point_prebuilt_slice_kernel_wrapper", dev, case.b, n, case.s, k, q.data_ptr(), idx.data_ptr(),
                  dist.data_ptr(), ws.data_ptr(), first, built_b)
    else:
        _lib.call("knn_point_prebuilt_kernel_wrapper", dev, case.b, n, case.s, k, q.data_ptr(), idx.data_ptr(), dist.data_ptr(),
                  ws.data_ptr())
    return dist, idx


def oracle(case, xyz, new_xyz):
    from oracle import ops as O
    first = 1 if case.entry == "slice" else 0
    return O.knn_point_with_dist(case.k, xyz[first:first + case.b].contiguous(), new_xyz[first:first + case.b].contiguous())


def differences(got, want):
    """Number of (query, rank) entries whose index or key differs; got on the device, want on the CPU."""
    d, i = got
    d_ref, i_ref = want
    return int((i.cpu() != i_ref).sum()), int((d.cpu().view(torch.int32) != d_ref.view(torch.int32)).sum())


def _rows0_main():
    """Child of test_pruned_kernel_serves_k_up_to_32_with_rows_off: this process was started with PWCLO_KNN_ROWS=0."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    if os.environ.get("PWCLO_KNN_ROWS") != "0":
        print("PWCLO_KNN_ROWS=0 is not set")
        return 2
    dev = torch.device("cuda:0")
    bad = 0
    for case in ROWS0_CASES:
        plan = plan_of(case)                          # use_rows=None: the switch as the launcher reads it
        if instantiations(plan) != case.want or plan["kernel"] != "pruned":
            print("%s: plan %r does not select the pruned kernel" % (case.name, plan))
            return 3
        xyz, new_xyz = make_inputs(case)
        want = oracle(case, xyz, new_xyz)
        di, dd = differences(run(case, xyz, new_xyz, dev), want)
        ei, ed = differences(run(case, xyz, new_xyz, dev, exhaustive=True), want)
        print("%s: pruned differs from the oracle at %d indices, %d keys; exhaustive at %d, %d" % (case.name, di, dd, ei, ed))
        bad += di + dd + ei + ed
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1:] == ["--rows0"]:
        sys.exit(_rows0_main())
    sys.exit("usage: knn_cases.py --rows0")
