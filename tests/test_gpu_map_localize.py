"""The map localiser on the GPU against the NumPy model of tests/map_localize_model.py: the index, the
ranks, counts and fp32 distances bit for bit, the planes at the tolerance the knn refiner's normals are held to, the sums
and the solve teacher-forced, the whole localiser on the box room, and a stale index after a rebuild."""
import functools

import numpy as np
import pytest
import torch

import icp_model as icp
import map_localize_cases as C
import map_localize_model as M
from pwclonet_pylidarslam_amd import _lib, map_localize
from pwclonet_pylidarslam_amd.global_map import GlobalMap
from pwclonet_pylidarslam_amd.map_localize import MapLocalizer

pytestmark = pytest.mark.gpu
F = np.float32


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _device_map(dev, clouds, poses, v, capacity=None):
    """clouds (S, K, n, 3), poses (S, K, 4, 4) -> a GlobalMap of S streams that holds the K keyframes."""
    S, K, n = clouds.shape[:3]
    gm = GlobalMap(S, n, v, max_keyframes=K, capacity=capacity, graph=False, device=dev)
    X = _dev(np.ascontiguousarray(np.transpose(poses, (1, 0, 2, 3))), dev)
    for k in range(K):
        gm.advance(_dev(clouds[:, k], dev), [k] * S, X)
    return gm, X


def _ops_args(gm):
    b = gm.bufs
    return b["keys"], b["rows"], b["points"], b["source"], gm.totals()


def _host(gm, s, idx=None):
    """Stream s of a device map as the model takes it: (keys, index, points, source, M, v)."""
    b = gm.bufs
    m = min(int(gm.totals()[s]), gm.capacity)
    keys = b["keys"][s].cpu().numpy().view(np.uint64)
    return (keys, None if idx is None else idx[s].cpu().numpy(), b["points"][s, :m].cpu().numpy(), b["source"][s, :m].cpu().numpy(),
            m, gm.voxel_size)


def _with_index(args, idx):
    return (args[0], idx) + args[2:]


@functools.lru_cache(maxsize=None)
def _maps(S, K, n, v):
    made = [C.random_map(K, n, v, seed=7 + s) for s in range(S)]
    return np.stack([m[0] for m in made]), np.stack([m[1] for m in made])


# ---- 1. the index ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [1, 255, 256, 257, None])
def test_index_equals_the_model(cuda, cap):
    clouds, poses = _maps(2, 3, 300, 0.3)
    gm, _ = _device_map(cuda, clouds, poses, 0.3, capacity=cap)
    assert cap is None or int(gm.totals().min()) > cap                   # dropped winners get no rank
    idx, indexed = map_localize.index(*_ops_args(gm), 0.3)
    for s in range(2):
        h = _host(gm, s)
        want = M.index(h[0], h[2], h[4], 0.3)
        assert np.array_equal(idx[s].cpu().numpy(), want) and int(indexed[s]) == h[4] == (want >= 0).sum()
    _lib.synchronize(cuda)


def test_full_index_equals_appended_passes_and_the_marker_goes_to_slot_T(cuda):
    clouds, poses = _maps(2, 3, 96, 0.3)
    S, K, n = clouds.shape[:3]
    gm = GlobalMap(S, n, 0.3, max_keyframes=K, graph=False, device=cuda)
    loc = MapLocalizer(gm, graph=False)
    X = _dev(np.ascontiguousarray(np.transpose(poses, (1, 0, 2, 3))), cuda)
    for k in range(K):
        gm.advance(_dev(clouds[:, k], cuda), [k] * S, X)
        loc.index(full=False)
        assert loc.indexed().tolist() == gm.totals().tolist()
    full, _ = map_localize.index(*_ops_args(gm), 0.3)
    assert torch.equal(loc.bufs["index"], full)
    c = [c for c in C.table() if c["name"] == "marker"][0]
    gm, _ = _device_map(cuda, c["clouds"][None], c["poses"][None], c["v"])
    idx, _ = map_localize.index(*_ops_args(gm), c["v"])
    T = gm.bufs["keys"].shape[1]
    assert int(idx[0, T]) == 0 and (idx[0] >= 0).sum() == 2
    _lib.synchronize(cuda)


# ---- 2. the lookup -----------------------------------------------------------------------------------------------------

def _check_lookup(gm, idx, q, R, got, active=None, newest=None):
    rank, count, dist = (g.cpu().numpy() for g in got)
    for s in range(q.shape[0]):
        if active is not None and not active[s]:
            assert (rank[s] == -1).all() and (count[s] == 0).all() and np.isinf(dist[s]).all()      # untouched
            continue
        want = M.lookup(*_host(gm, s, idx), q[s], R, newest=None if newest is None else int(newest[s]))
        assert np.array_equal(rank[s], want[0]) and np.array_equal(count[s], want[1]), s
        assert np.array_equal(_bits(dist[s]), _bits(want[2])), s
    return rank, count, dist


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("v", [0.3, 1.0])
def test_lookup_equals_the_model(cuda, n, R, v):
    S = 2
    clouds, poses = _maps(S, 3, 128, v)
    gm, _ = _device_map(cuda, clouds, poses, v)
    idx, _ = map_localize.index(*_ops_args(gm), v)
    q = np.stack([C.queries(_host(gm, s)[2], n, v, R, seed=5 + s) for s in range(S)])
    got = map_localize.lookup(*_ops_args(gm), idx, v, _dev(q, cuda), R)
    rank, count, dist = _check_lookup(gm, idx, q, R, got)
    if n >= 255:
        assert (rank >= 0).mean() > 0.3 and (rank == -1).any() and (dist == 0).any() and count.max() > 5
    again = map_localize.lookup(*_ops_args(gm), idx, v, _dev(q, cuda), R)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    _lib.synchronize(cuda)


@pytest.mark.parametrize("S", [1, 33])
def test_lookup_with_scattered_streams_and_a_source_gate(cuda, S):
    n, v, R = 257, 0.3, 1
    clouds, poses = _maps(S, 2, 64, v)
    gm, _ = _device_map(cuda, clouds, poses, v)
    idx, _ = map_localize.index(*_ops_args(gm), v)
    q = np.stack([C.queries(_host(gm, s)[2], n, v, R, seed=5 + s) for s in range(S)])
    active = np.array([1 if (s % 3 != 1 or S == 1) else 0 for s in range(S)], dtype=np.int32)
    q[active == 0] = np.nan                                             # an idle stream's rows are never read
    newest = np.array([s % 2 for s in range(S)], dtype=np.int32)        # frames 0..1: half the streams see keyframe 0 only
    got = map_localize.lookup(*_ops_args(gm), idx, v, _dev(q, cuda), R, _dev(newest, cuda), _dev(active, cuda))
    _check_lookup(gm, idx, q, R, got, active, newest)
    src = gm.bufs["source"].cpu().numpy()
    rank = got[0].cpu().numpy()
    for s in np.flatnonzero((newest == 0) & (active == 1)):
        assert (src[s, rank[s][rank[s] >= 0], 0] == 0).all()
    _lib.synchronize(cuda)


# ---- 3. the planted cases, planes ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", C.table(), ids=lambda c: c["name"])
def test_planted_case_equals_the_model(cuda, c):
    gm, _ = _device_map(cuda, c["clouds"][None], c["poses"][None], c["v"])
    idx, _ = map_localize.index(*_ops_args(gm), c["v"])
    partial, rank, count, dist, normal = map_localize.accumulate(
        *_ops_args(gm), idx, c["v"], _dev(c["q"][None], cuda), None, c["R"], 0.5, c["max_dist"], c["min_neighbours"], nearest=True)
    row, mag, near = M.accumulate(*_host(gm, 0, idx), c["q"], None, c["R"], 0.5, c["max_dist"], c["min_neighbours"])
    assert np.array_equal(rank[0].cpu().numpy(), near["rank"]) and np.array_equal(count[0].cpu().numpy(), near["count"])
    assert np.array_equal(_bits(dist[0].cpu().numpy()), _bits(near["dist"]))
    got = normal[0].cpu().numpy()
    assert np.array_equal((got != 0).any(axis=1), near["pair"])          # the zero-pair decision, exactly
    assert float(partial[0].sum(dim=0)[M.PAIRS]) == row[M.PAIRS] == near["pair"].sum()
    if near["pair"].any():
        assert np.abs(np.abs(got[near["pair"]]) - np.abs(near["normal"][near["pair"]])).max() <= 2.0 ** -23
    _lib.synchronize(cuda)


@pytest.mark.parametrize("R, v", [(1, 0.3), (2, 0.3), (1, 1.0)])
def test_planes_against_the_model(cuda, R, v):
    """The bound of test_gpu_icp.test_normals_against_the_model: 1 - |n . n_model| <= 64 eps64 / gap for the points whose
    relative eigen-gap is at least GAP_MIN, at most GAP_CAP of the planes left out."""
    clouds, poses = _maps(1, 3, 300, v)
    gm, _ = _device_map(cuda, clouds, poses, v)
    idx, _ = map_localize.index(*_ops_args(gm), v)
    h = _host(gm, 0, idx)
    q = C.queries(h[2], 513, v, R)
    t = np.array([0.5, -0.25, 2.0])
    T = icp.pose(np.eye(3), t)
    p = (q.astype(np.float64) - t).astype(F)
    md = M.largest_max_dist(R, v)
    _, rank, count, dist, normal = map_localize.accumulate(*_ops_args(gm), idx, v, _dev(p[None], cuda), _dev(T[None], cuda),
                                                           R, 0.5, md, 5, nearest=True)
    qq = M.gm.world(p, T)
    usable, cand = M.candidates(*h, qq, R)
    best, cnt, d = M.nearest(h[2], qq, cand)
    assert np.array_equal(rank[0].cpu().numpy(), best) and np.array_equal(count[0].cpu().numpy(), cnt)
    fit = usable & (best >= 0) & (cnt >= 5) & (d <= F(md))
    assert fit.sum() > 150
    want, val, gap = M.planes(h[2], cand[fit], best[fit], t)
    g = normal[0].cpu().numpy().astype(np.float64)
    assert not g[~fit].any() and np.array_equal((g[fit] != 0).any(axis=1), (want != 0).any(axis=1))
    has = (want != 0).any(axis=1)
    use = has & (gap >= icp.GAP_MIN)
    assert (has & ~use).sum() <= icp.GAP_CAP * has.sum()
    gg = g[fit][use]
    length = np.linalg.norm(gg, axis=1)
    assert (np.abs(length - 1.0) <= 2.0 ** -23).all()
    miss = 1.0 - np.abs(np.einsum("ni,ni->n", gg / length[:, None], want[use]))
    ratio = miss / (64.0 * icp.EPS64 / gap[use])
    print("planes R=%d v=%g: %d fitted, worst miss / bound = %.3g" % (R, v, use.sum(), ratio.max()))
    assert (ratio <= 1.0).all()
    y = h[2][best[fit]][use].astype(np.float64)
    assert (np.einsum("ni,ni->n", gg, y - t) <= 0.0).all()               # towards the sensor
    _lib.synchronize(cuda)


# ---- 4. sums and solve, teacher-forced; the whole localiser ----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _scene():
    return C.scene()


def _scene_map(dev, S):
    s = _scene()
    clouds = np.repeat(s["clouds"][None], S, axis=0)
    poses = np.repeat(s["poses"][None], S, axis=0)
    return s, _device_map(dev, clouds, poses, s["v"])[0]


def test_accumulate_and_solve_against_the_model(cuda):
    S, iters, R = 2, 4, C.SCENE_RADIUS
    s, gm = _scene_map(cuda, S)
    loc = MapLocalizer(gm, iters=iters, radius=R, graph=False)
    loc.index()
    cloud = np.repeat(s["cloud"][None], S, axis=0)
    init = np.stack(s["guesses"])
    T, steps = loc.localize(_dev(cloud, cuda), _dev(init, cuda), trace=True)
    moved = 0
    for st in range(S):
        h, status = _host(gm, st, loc.bufs["index"]), 0
        for it, step in enumerate(steps):
            Tb = step["T_before"][st].cpu().numpy()
            row, mag, near = M.accumulate(*h, cloud[st], Tb, R, 0.5, loc.max_dist, 5, normals=step["normal"][st].cpu().numpy())
            got = step["sum"][st].cpu().numpy()
            assert np.array_equal(step["rank"][st].cpu().numpy(), near["rank"]) and got[M.PAIRS] == row[M.PAIRS]
            assert np.array_equal(_bits(step["dist"][st].cpu().numpy()), _bits(near["dist"]))
            assert (np.abs(got - row) <= 1e-12 * mag + 1e-300).all(), (st, it)
            want = icp.solve(got, Tb, status, it, 1e-6, 1e-4, 64)
            status = want["status"]
            assert int(step["status"][st]) == status
            assert np.abs(step["delta"][st].cpu().numpy() - want["delta"]).max() <= 1e-10
            assert np.abs(step["T"][st].cpu().numpy() - want["T"]).max() <= 1e-10
            moved += int(np.abs(want["delta"]).max() > 0)
    assert moved >= 2 * S
    _lib.synchronize(cuda)


def test_localizer_on_the_box_room(cuda):
    S, R = 2, C.SCENE_RADIUS
    s, gm = _scene_map(cuda, S)
    cloud, init = _dev(np.repeat(s["cloud"][None], S, axis=0), cuda), _dev(np.stack(s["guesses"]), cuda)
    eager, graphed = MapLocalizer(gm, radius=R, graph=False), MapLocalizer(gm, radius=R, graph=True)
    outs = []
    for loc, calls in ((eager, 1), (graphed, 3)):
        loc.index()
        for _ in range(calls):
            outs.append(loc.localize(cloud, init).clone())
    assert all(torch.equal(outs[0], o) for o in outs[1:])                # eager = first call = replay = second replay
    assert graphed.captures == 1 and eager.captures == 0
    T = outs[0].cpu().numpy()
    for st in range(S):
        h = _host(gm, st, eager.bufs["index"])
        Tm, status, _ = M.localize(*h, s["cloud"], s["guesses"][st], R=R)
        dev_err, model_err = icp.pose_error(T[st], s["truth"]), icp.pose_error(Tm, s["truth"])
        print("stream %d: device error %.3g, model error %.3g, guess %.3g" % (st, dev_err, model_err,
                                                                             icp.pose_error(s["guesses"][st], s["truth"])))
        assert dev_err <= 1.5 * model_err
    assert (eager.diagnostics()["pairs"] >= 64).all()
    # an idle stream keeps its pose word for word
    keep = graphed.bufs["T"].clone()
    graphed.localize(cloud, init.flip(0).contiguous(), active=[1, 0])
    assert torch.equal(graphed.bufs["T"][1], keep[1]) and graphed.status().tolist()[1] == 8 and graphed.captures == 1
    _lib.synchronize(cuda)


# ---- 5. a rebuild under a stale index ------------------------------------------------------------------------------------

def test_after_a_rebuild_lookups_are_correct_or_empty_until_the_next_index(cuda):
    s = C.stale()
    v, K = s["v"], 3
    gm, _ = _device_map(cuda, s["clouds"][None], s["before"][None], v)
    idx, _ = map_localize.index(*_ops_args(gm), v)
    gm.rebuild(_dev(s["after"][:, None], cuda))
    h = _host(gm, 0, idx)
    fresh = M.index(h[0], h[2], h[4], v)
    for R in (1, 2):
        got = [g[0].cpu().numpy() for g in map_localize.lookup(*_ops_args(gm), idx, v, _dev(s["q"][None], cuda), R)]
        stale_want = M.lookup(*h, s["q"], R)
        assert np.array_equal(got[0], stale_want[0]) and np.array_equal(_bits(got[2]), _bits(stale_want[2]))
        _, cand = M.candidates(*h, s["q"], R)
        _, ref = M.candidates(*_with_index(h, fresh), s["q"], R)
        assert ((cand == ref) | (cand == -1)).all() and (cand != ref).any() and (cand >= 0).any()
    map_localize.index(*_ops_args(gm), v, index=idx)
    assert np.array_equal(idx[0].cpu().numpy(), M.index(h[0], h[2], h[4], v, out=h[1].copy()))
    for R in (1, 2):
        got = [g[0].cpu().numpy() for g in map_localize.lookup(*_ops_args(gm), idx, v, _dev(s["q"][None], cuda), R)]
        want = M.lookup(*_with_index(h, idx[0].cpu().numpy()), s["q"], R)
        ref = M.lookup(*_with_index(h, fresh), s["q"], R)
        assert all(np.array_equal(a, b) for a, b in zip(want, ref))      # a full pass over a stale index hides nothing
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(_bits(got[2]), _bits(want[2]))
    _lib.synchronize(cuda)
