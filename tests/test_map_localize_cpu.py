"""The map localiser, the parts that need no GPU: the NumPy model of tests/map_localize_model.py
against a brute-force nearest, the two properties of the index, the planted cases and their faults, the scene on which the
fp64 model must converge, the ABI's new names, the byte formula and the host's refusals."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import global_map_model as GM            # noqa: E402
import icp_model as icp                  # noqa: E402
import map_localize_cases as C           # noqa: E402
import map_localize_model as M           # noqa: E402
from pwclonet_pylidarslam_amd import _lib, global_map, map_localize      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ---- lookup ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("v", [0.3, 1.0])
def test_lookup_is_the_brute_force_nearest_within_the_block(R, v):
    clouds, poses = C.random_map(3, 128, v)
    mp = M.Map(clouds, poses, v)
    assert mp.M > 150
    q = C.queries(mp.points, 257, v, R)
    rank, count, dist = M.lookup(*mp.args(), q, R)
    ok = np.isfinite(q).all(axis=1) & (np.abs(q) < 1e30).all(axis=1)
    brute, who = M.brute_nearest(mp.points, q[ok])
    # a map point nearer than (R - 2^-20) v lies inside the block whatever the rounding of the two divisions does
    near = brute <= F((R - 2.0 ** -20) * v)
    assert near.sum() > 60
    assert np.array_equal(_bits(dist[ok][near]), _bits(brute[near]))
    assert np.array_equal(_bits(mp.points[rank[ok][near]]), _bits(mp.points[who[near]]))
    inside = np.isfinite(dist[ok])                                       # whatever the block returns is a map point at that distance
    assert (dist[ok][inside] >= brute[inside]).all()
    assert (rank[~ok] == -1).all() and (count[~ok] == 0).all() and np.isinf(dist[~ok]).all()
    assert (rank[ok][~np.isfinite(dist[ok])] == -1).all() and (count <= (2 * R + 1) ** 3).all()


def test_vectorised_slots_equal_the_probe():
    clouds, poses = C.random_map(3, 128, 0.3)
    mp = M.Map(clouds, poses, 0.3, T=512)                               # a crowded table: probes past the home slot
    cand, h = GM.keys(mp.points, 0.3)
    other = M.voxel_key(np.random.default_rng(1).integers(-50, 50, (300, 3)))
    hs = np.concatenate([h, other, [M.EMPTY]])
    assert np.array_equal(M._slots(mp.keys, hs), [M.probe(mp.keys, x) for x in hs])
    assert any(M.home(x, 512) != M.probe(mp.keys, x) for x in h)


# ---- the index ---------------------------------------------------------------------------------------------------------

def test_full_index_equals_appended_passes():
    clouds, poses = C.random_map(5, 96, 0.3)
    T = M.table_slots(5 * 96)
    idx, lo = np.full(T + 1, -1, dtype=np.int32), 0
    for k in range(1, 6):
        pts, _, total = GM.build(clouds[:k], poses, 0.3)
        keys = M.table(pts, 0.3, T)                                     # a later keyframe only appends: the same slots
        M.index(keys, pts, total, 0.3, out=idx, lo=lo)
        lo = total
    full = M.index(keys, pts, total, 0.3)
    assert np.array_equal(idx, full) and (full >= 0).sum() == total
    capped = M.index(keys, pts[:100], 100, 0.3)                         # winners past the capacity get no rank
    assert (capped >= 0).sum() == 100 and capped.max() == 99


def test_a_stale_index_yields_the_new_maps_point_or_nothing():
    s = C.stale()
    old = M.Map(s["clouds"], s["before"], s["v"])
    new = M.Map(s["clouds"], s["after"], s["v"], T=old.T)
    assert not np.array_equal(old.keys, new.keys)
    args = (new.keys, old.index, new.points, new.source, new.M, s["v"])
    for R in (1, 2):
        want = M.lookup(*new.args(), s["q"], R)
        _, got = M.candidates(*args, s["q"], R)
        _, ref = M.candidates(*new.args(), s["q"], R)
        assert ((got == ref) | (got == -1)).all()                       # every candidate is the new map's, or hidden
        assert (got != ref).any() and (got >= 0).any()
        _, wrong = M.candidates(*args, s["q"], R, fault="no_validation")
        assert ((wrong != ref) & (wrong >= 0)).any()                    # without the validation: another voxel's point
        again = M.lookup(new.keys, M.index(new.keys, new.points, new.M, s["v"], out=old.index.copy()), new.points,
                         new.source, new.M, s["v"], s["q"], R)
        assert all(np.array_equal(a, b) for a, b in zip(again, want))   # after a full pass over the stale index


def test_max_source_frame_hides_exactly_the_later_frames():
    clouds, poses = C.random_map(4, 96, 0.3)
    mp = M.Map(clouds, poses, 0.3, frames=[0, 5, 10, 15])
    q = C.queries(mp.points, 128, 0.3, 1)
    for newest in (-1, 0, 7, 10, 99):
        keep = mp.source[:, 0] <= newest
        _, got = M.candidates(*mp.args(), q, 1, newest=newest)
        _, ref = M.candidates(*mp.args(), q, 1)
        assert np.array_equal(got, np.where((ref >= 0) & keep[np.maximum(ref, 0)], ref, -1))
    assert (M.candidates(*mp.args(), q, 1, newest=-1)[1] == -1).all()


# ---- the planted cases -------------------------------------------------------------------------------------------------

def _run(c, fault=None):
    mp = M.Map(c["clouds"], c["poses"], c["v"])
    row, _, near = M.accumulate(*mp.args(), c["q"], None, c["R"], 0.5, c["max_dist"], c["min_neighbours"], fault=fault)
    return mp, row, near


@pytest.mark.parametrize("c", C.table(), ids=lambda c: c["name"])
def test_case_reaches_its_edge_and_differs_under_its_fault(c):
    mp, row, near = _run(c)
    edge = c["edge"]
    if edge == "tie":
        _, rank = M.candidates(*mp.args(), c["q"], c["R"])
        d = M.nearest(mp.points, c["q"], rank)[2]
        hit = rank[0][rank[0] >= 0]
        assert len(hit) == 2 and hit[0] == near["rank"][0] == 0         # the first in order is the first point of the cloud
        e = c["q"][0] - mp.points[hit]
        assert len({float(np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2], dtype=F)) for x in e}) == 1 and d[0] > 0
    elif edge == "max_dist":
        assert near["dist"].tolist() == [float(x) for x in c["q"][:, 2]] and near["pair"].tolist() == [True, True, False]
        assert near["count"].tolist() == [9, 9, 9] and row[M.PAIRS] == 2.0
        assert np.array_equal(np.abs(near["normal"][:2]), [[0, 0, 1]] * 2)
    elif edge == "count_eq":
        assert near["count"].tolist() == [5] and near["pair"].tolist() == [True] and row[M.PAIRS] == 1.0
    elif edge == "count_below":
        assert near["count"].tolist() == [4] and near["pair"].tolist() == [False] and not near["normal"].any()
    elif edge == "collinear":
        assert near["count"].tolist() == [5] and near["dist"][0] == F(0.25) and not near["normal"].any() and row[M.PAIRS] == 0
    elif edge == "single":
        assert near["count"].tolist() == [1] and near["rank"].tolist() == [0] and not near["normal"].any() and row[M.PAIRS] == 0
    elif edge == "unusable":
        assert near["rank"].tolist() == [-1] * 5 and near["count"].tolist() == [0] * 5 and np.isinf(near["dist"]).all()
    elif edge == "range":
        with np.errstate(all="ignore"):
            cc = np.rint(c["q"].astype(np.float64) / c["v"]).astype(np.int64)
        assert cc[:, 0].tolist() == [2 ** 31 - 1, -(2 ** 31 - 1)]
        assert near["rank"].tolist() == [0, 1] and near["count"].tolist() == [1, 1] and near["dist"].tolist() == [0.0, 0.0]
        nb = cc[:, None, :] + M.offsets(1)[None]
        assert (np.abs(nb) >= 2 ** 31).any(axis=2).sum() == 18         # nine voxels past the limit on either side
    elif edge == "marker":
        assert M.voxel_key(np.array(C.MARKER)) == M.EMPTY
        assert mp.index[mp.T] == 0 and near["rank"].tolist() == [0, 1] and near["count"].tolist() == [2, 2]
    else:
        raise AssertionError(edge)
    if c["fault"] == "no_range_skip":
        # A neighbour past 2^31 can only be seen through a map voxel with the same 64-bit hash, and none was constructed:
        # what the fault changes is which keys are asked for, and that is all that is compared.  THIS EDGE IS THEREFORE
        # NOT VERIFIED ON THE DEVICE: a kernel that looked those neighbours up would pass every test of this project.
        (_, h, ask), (_, fh, fask) = M.asked(c["v"], c["q"], c["R"]), M.asked(c["v"], c["q"], c["R"], c["fault"])
        assert np.array_equal(h, fh) and (~ask).sum() == 18 and fask.all()
    elif c["fault"] is not None:
        _, frow, fnear = _run(c, c["fault"])
        same = all(np.array_equal(near[k], fnear[k]) for k in ("rank", "count", "pair")) and np.array_equal(row, frow)
        assert not same, c["fault"]


def test_a_distance_that_overflows_still_names_a_candidate():
    rank = np.array([[-1, 1, 0], [-1, -1, -1]])
    pts = np.array([[3e19, 0, 0], [-3e19, 0, 0]], dtype=F)
    best, count, dist = M.nearest(pts, np.zeros((2, 3), dtype=F), rank)
    assert best.tolist() == [1, -1] and count.tolist() == [2, 0] and np.isinf(dist).all()


def test_the_module_and_the_model_agree_on_the_largest_max_dist():
    for R in (1, 2):
        for v in (0.3, 1.0, 0.1, 0.7, 1e-3, 123.456, C.EDGE_V):
            a, b = map_localize.largest_max_dist(R, v), M.largest_max_dist(R, v)
            assert a == b and a <= R * v < float(np.nextafter(F(a), F(np.inf)))


def test_every_fault_has_a_case():
    assert {c["fault"] for c in C.table()} | {"no_validation"} >= set(M.FAULTS)


# ---- the scene ---------------------------------------------------------------------------------------------------------

def test_the_fp64_model_converges_on_the_box_room():
    """Keyframes of the section 21 box room at their true poses, v = 0.3; guesses off by 2 degrees and 0.3 m.  The condition
    (final error at most a quarter of the guess's) is on the scene.  It fails at radius 1, where max_dist = 0.3 m is no more
    than the guess's own error and too few points find a partner; it holds at radius 2 (max_dist = 0.6 m), which is
    the radius recorded in map_localize_cases.SCENE_RADIUS and used by the GPU test."""
    s = C.scene()
    mp = M.Map(s["clouds"], s["poses"], s["v"])
    ratios = {}
    for R in (1, 2):
        ratios[R] = []
        for g in s["guesses"]:
            T, status, steps = M.localize(*mp.args(), s["cloud"], g, R=R)
            ratios[R].append(icp.pose_error(T, s["truth"]) / icp.pose_error(g, s["truth"]))
    print("final error / guess error per radius:", ratios)
    assert C.SCENE_RADIUS in ratios and max(ratios[C.SCENE_RADIUS]) <= 0.25


# ---- declarations and host logic ---------------------------------------------------------------------------------------

NEW = [("map_index_kernel_wrapper", 13), ("map_localize_begin_kernel_wrapper", 4),
       ("map_localize_accumulate_kernel_wrapper", 24)]


@pytest.mark.parametrize("name, arity", NEW)
def test_new_symbols_are_declared_with_the_header_arity(name, arity):
    with open(os.path.join(ROOT, "include", "pwclo_ops.h")) as f:
        header = f.read()
    args, res = _lib.SIGNATURES[name]
    m = re.search(r"void\s+%s\s*\(([^)]*)\)\s*;" % name, header)
    assert m is not None and res is None
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(args) == len(params) == arity
    for p, a in zip(params, args):
        want = _lib._F if "*" in p else ctypes.c_float if p.startswith("float") else ctypes.c_double if p.startswith("double") \
            else ctypes.c_longlong if p.startswith("long long") else _lib._i
        assert a is want, (name, p, a)
    assert hasattr(_lib.load(), name) and "13. localisation in the global map" in header


def test_index_bytes_and_the_version():
    lib = _lib.load()
    assert lib.pwclo_abi_version() == 1
    for S, T in ((1, 64), (8, 1 << 24), (1024, 1 << 10), (3, 1 << 30)):
        assert lib.map_localize_index_bytes(S, T) == map_localize.index_bytes(S, T) == 4 * S * (T + 1)
    assert map_localize.index_bytes(1, global_map.table_slots(1024, 8192)) == 4 * ((1 << 24) + 1)      # 67 MB at the default bank
    for bad in ((0, 64), (1025, 64), (1, 32), (1, 96), (1, 1 << 31)):
        assert lib.map_localize_index_bytes(*bad) == 0


def test_host_refusals():
    gm = global_map.GlobalMap(streams=2, num_points=64, voxel_size=0.3)
    make = lambda **kw: map_localize.MapLocalizer(gm, **kw)
    for kw in (dict(radius=0), dict(radius=3), dict(radius=1.0), dict(radius=True), dict(max_dist=0.31), dict(max_dist=-0.1),
               dict(radius=2, max_dist=0.61), dict(max_dist=float("nan")), dict(iters=0), dict(sigma=0.0), dict(min_neighbours=0),
               dict(min_neighbours=2.5), dict(min_pairs=0), dict(damping=-1.0)):
        with pytest.raises(ValueError, match="MapLocalizer"):
            make(**kw)
    with pytest.raises(ValueError, match="GlobalMap"):
        map_localize.MapLocalizer(object())
    loc = make()
    assert loc.max_dist <= 0.3 < float(np.nextafter(F(loc.max_dist), F(1))) and make(radius=2, max_dist=0.6).max_dist <= 0.6
    assert loc.status() is None and loc.diagnostics() is None and loc.indexed() is None and loc.captures == 0
    cloud, init = torch.zeros(2, 64, 3), torch.eye(4, dtype=torch.float64).expand(2, 4, 4).contiguous()
    with pytest.raises(ValueError, match="no buffers yet"):
        loc.index()
    with pytest.raises(RuntimeError, match="CPU not supported"):
        loc.localize(cloud, init)
    for args, kw in (((cloud.double(), init), {}), ((cloud[:1], init), {}), ((cloud, init.float()), {}), ((cloud, init[:1]), {}),
                     ((cloud, init), dict(active=[1])), ((cloud, init), dict(max_source_frame=[1])),
                     ((cloud, init), dict(max_source_frame=[0.5, 1.0])),
                     ((cloud, init), dict(max_source_frame=torch.zeros(2, dtype=torch.int64))), ((cloud, init), dict(trace=True))):
        with pytest.raises(ValueError, match="MapLocalizer"):
            loc.localize(*args, **kw)
    assert loc.bufs is None
    # the ops: shapes and kinds are refused on the host, before a launch
    S, T, cap = 2, 64, 8
    mk = dict(keys=torch.zeros(S, T, dtype=torch.int64), rows=torch.zeros(S, T + 2, dtype=torch.int32),
              points=torch.zeros(S, cap, 3), source=torch.zeros(S, cap, 2, dtype=torch.int32),
              total=torch.zeros(S, dtype=torch.int32), index=torch.zeros(S, T + 1, dtype=torch.int32))
    q = torch.zeros(S, 5, 3)
    call = lambda q=q, radius=1, **kw: map_localize.lookup(*[dict(mk, **kw)[k] for k in ("keys", "rows", "points", "source",
                                                                                          "total", "index")], 0.3, q, radius)
    for kw in (dict(keys=mk["keys"][:, :48].contiguous()), dict(keys=mk["keys"].int()), dict(rows=mk["rows"][:, :T].contiguous()),
               dict(points=mk["points"].double()), dict(source=mk["source"][:, :4].contiguous()),
               dict(total=mk["total"].long()), dict(index=mk["index"][:, :T].contiguous()), dict(radius=3),
               dict(q=q.double()), dict(q=q[:1]), dict(keys=torch.zeros(1025, T, dtype=torch.int64))):
        with pytest.raises(ValueError, match="map_localize"):
            call(**kw)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        call()
    with pytest.raises(ValueError, match="max_dist"):
        map_localize.accumulate(*[mk[k] for k in ("keys", "rows", "points", "source", "total", "index")], 0.3, q, None,
                                max_dist=0.31)


def test_library_refusals():
    lib = _lib.load()
    one = ctypes.c_void_p(256)                                           # an aligned non-null address that is never read
    ok = [1, 5, 64, 8, 0.3, 1, one, one, one, one, 1, one, one, None, None, 0.5, 0.25, 5, one, None, None, None, None, None]
    bad = {0: 0, 1: 0, 2: 96, 3: 0, 4: 0.0, 5: 3, 6: None, 10: 0, 11: None, 12: None, 15: 0.0, 16: 0.31, 17: 0, 18: None,
           19: one}
    for at, value in bad.items():
        args = list(ok)
        args[at] = value
        lib.pwclo_clear_error()
        lib.map_localize_accumulate_kernel_wrapper(*args)
        assert lib.pwclo_last_error() != 0, at
        assert b"map_localize_accumulate" in lib.pwclo_last_error_message()
    lib.pwclo_clear_error()
    lib.map_index_kernel_wrapper(1, 64, 8, 0.3, one, one, one, one, 1, 1, None, None, one)
    assert lib.pwclo_last_error() != 0
    lib.pwclo_clear_error()
    lib.map_localize_begin_kernel_wrapper(1025, one, None, one)
    assert lib.pwclo_last_error() != 0
    lib.pwclo_clear_error()
