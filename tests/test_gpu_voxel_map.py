"""The persistent voxel map on the GPU: insertion and lookup bit for bit against the NumPy model of
tests/voxel_map_model.py, the sums and the solve against its fp64 rows, the whole refiner on icp_model's box room, masks
against lock-step refiners of the streams' own, and the keyframe gate."""
import functools

import numpy as np
import pytest
import torch

import icp_mask_model as masked
import icp_model as model
import keyframe_model as kf
import voxel_map_model as vm
from pwclonet_pylidarslam_amd import _lib, voxel_map

pytestmark = pytest.mark.gpu


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    t = t.contiguous()
    return t.view({8: torch.int64, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _grid_is(sec, s, g):
    """A device grid's stream s holds the model grid's bits, section by section."""
    ok = np.array_equal(sec["coord"][s].cpu().numpy(), g.coord) and np.array_equal(sec["keys"][s].cpu().numpy(), g.keys)
    for name, want in (("points", g.points), ("normals", g.normals)):
        ok = ok and np.array_equal(sec[name][s].cpu().numpy().view(np.int32), want.view(np.int32))
    return ok


# ---- 1. insertion --------------------------------------------------------------------------------------------------------------

INSERT_CASES = [(1, 256, (8, 8, 4), 0.5, 1.1), (2, 300, (16, 16, 8), 1.0, 4.3), (33, 300, (8, 8, 4), 1.0, 2.3)]


def _insert_run(dev, S, n, extent, voxel, step, frames=5):
    data = [vm.walk_clouds(10 + s, frames, n, step, 0.45 * voxel * extent[0]) for s in range(S)]
    r = np.random.default_rng([S, n])
    grid = voxel_map.new_grid(S, extent, dev)
    sec = voxel_map.sections(grid, S, extent)
    P = torch.zeros((S, 4, 4), dtype=torch.float64, device=dev)
    nonempty = torch.zeros((S, 1), dtype=torch.int32, device=dev)
    seq = torch.zeros((S,), dtype=torch.int32, device=dev)
    models = [vm.Grid(extent, voxel) for _ in range(S)]
    for k in range(frames):
        active = np.ones((S,), dtype=np.int32) if S < 3 else (r.random(S) < 0.6).astype(np.int32)
        cloud = np.stack([d[0][k] for d in data])
        cloud[:, 5] = [np.nan, 0.0, 0.0]                            # a row that is no candidate
        cloud[:, 6] = [0.0, np.inf, 0.0]
        nrm = np.stack([d[1][k] for d in data])
        P.copy_(_dev(np.stack([d[2][k] for d in data]), dev))
        act = None if S < 3 else _dev(active, dev)
        slot = voxel_map.insert(grid, extent, voxel, _dev(cloud, dev), _dev(nrm, dev), P, seq, active=act)
        voxel_map.pose(P, nonempty, seq, active=act)
        for s in range(S):
            if active[s]:
                want = models[s].insert(cloud[s], nrm[s], data[s][2][k])
                models[s].seq += 1
                assert np.array_equal(slot[s].cpu().numpy(), want), (k, s)
            assert _grid_is(sec, s, models[s]), (k, s)              # idle streams keep their bits
            assert int(seq[s]) == models[s].seq and int(nonempty[s, 0]) == int(models[s].seq > 0)
    return grid, models


@pytest.mark.parametrize("S, n, extent, voxel, step", INSERT_CASES)
def test_insert_against_the_model_frame_by_frame(cuda, S, n, extent, voxel, step):
    grid, models = _insert_run(cuda, S, n, extent, voxel, step)
    again, _ = _insert_run(cuda, S, n, extent, voxel, step)
    assert torch.equal(grid, again)                                 # a second run: the same bits
    mp = models[0].map_points()
    assert len(mp["keys"]) > 50 and mp["voxels"][:, 0].max() >= extent[0]      # the walk went once round the torus
    _lib.synchronize(cuda)


# ---- 2. lookup -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S, n, extent, voxel, step", INSERT_CASES[:2])
def test_nearest_against_the_model(cuda, S, n, extent, voxel, step):
    grid, models = _insert_run(cuda, S, n, extent, voxel, step)
    r = np.random.default_rng(5)
    q = np.empty((S, n, 3), dtype=np.float32)
    period = np.float32(extent[0] * voxel)
    for s, g in enumerate(models):
        pts = g.map_points()["points"]
        base = pts[r.integers(0, len(pts), n)]
        q[s] = base + r.normal(0.0, 0.3 * voxel, (n, 3)).astype(np.float32)
        q[s, 0::7, 0] += period                                     # one torus period away: the cell aliases, the voxel differs
        q[s, 1::7] = r.uniform(-400.0, 400.0, (len(q[s, 1::7]), 3))  # empty neighbourhoods, far outside every box
        q[s, 2], q[s, 3], q[s, 4] = [np.nan, 0, 0], [0, -np.inf, 0], [3e38, 0, 0]
        q[s, 9] = base[9]                                           # a stored point itself: d = 0
    eye = torch.eye(4, dtype=torch.float64, device=cuda).expand(S, 4, 4).contiguous()
    cell, octant, dist = voxel_map.nearest(grid, extent, voxel, _dev(q, cuda), eye)
    kinds = set()
    for s, g in enumerate(models):
        wc, wo, wd = g.lookup(q[s])
        assert np.array_equal(cell[s].cpu().numpy(), wc) and np.array_equal(octant[s].cpu().numpy(), wo)
        assert np.array_equal(dist[s].cpu().numpy().view(np.int32), wd.view(np.int32))
        assert (wc[2:5] == -1).all() and wd[9] == 0.0
        brute = vm.brute_nearest(g, q[s])
        near = brute <= np.float32(voxel)
        assert np.array_equal(wd[near], brute[near])
        kinds |= {"alias-miss"} if (wc[0::7] == -1).any() else set()
        kinds |= {"empty"} if (wc[1::7] == -1).all() else set()
        kinds |= {"hit"} if near.sum() > n // 3 else set()
    assert kinds == {"alias-miss", "empty", "hit"}
    _lib.synchronize(cuda)


def test_the_pair_ends_at_max_dist_exactly(cuda):
    """d on both fp32 neighbours of max_dist: one stored point, queries along x at prev(1), 1 and next(1)."""
    extent, voxel, f = (8, 8, 4), 1.0, np.float32
    grid = voxel_map.new_grid(1, extent, cuda)
    eye = torch.eye(4, dtype=torch.float64, device=cuda)[None].contiguous()
    seq = torch.zeros((1,), dtype=torch.int32, device=cuda)
    cloud = np.tile(f([0.0, 0.25, 0.25]), (64, 1))
    nrm = np.tile(f([0.0, 0.0, 1.0]), (64, 1))
    slot = voxel_map.insert(grid, extent, voxel, _dev(cloud[None], cuda), _dev(nrm[None], cuda), eye, seq)
    assert slot.tolist() == [[0] * 64]                              # cell 0, octant 0; row 0 holds the key
    assert voxel_map.sections(grid, 1, extent)["keys"][0, 0].tolist() == [0] + [-1] * 7
    q = np.tile(f([100.0, 0.0, 0.0]), (64, 1))
    want = [np.nextafter(f(1), f(0)), f(1), np.nextafter(f(1), f(2))]
    for i, x in enumerate(want):                                    # the stored point has x = 0: d = |x| exactly
        q[i] = [x, 0.25, 0.25]
    partial, cell, octant, dist = voxel_map.accumulate(grid, extent, voxel, _dev(q[None], cuda), eye, max_dist=1.0,
                                                       nearest=True)
    assert dist[0, :3].tolist() == [float(w) for w in want] and cell[0, :4].tolist() == [0, 0, 0, -1]
    assert float(partial[0, 0, model.PAIRS]) == 2.0                 # d <= max_dist keeps prev(1) and 1, drops next(1)
    g = vm.Grid(extent, voxel)
    g.insert(cloud, nrm, np.eye(4))
    row, _, near = g.accumulate(q, np.eye(4), 0.5, 1.0, P=np.eye(4))
    assert row[model.PAIRS] == 2.0 and np.array_equal(near[2][:3], f(want))
    _lib.synchronize(cuda)


# ---- 3. sums and solve, teacher-forced -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n, extent, voxel", [(300, (16, 16, 8), 1.0), (256, (32, 32, 16), 0.5)])
def test_accumulate_and_solve_against_the_model(cuda, n, extent, voxel):
    S, frames, iters = 2, 3, 4
    rooms = [model.room(3 + s, frames, n) for s in range(S)]
    kw = dict(voxel_size=voxel, extent=extent, iters=iters, max_dist=voxel, min_pairs=32)
    ref = voxel_map.VoxelMapRefiner(S, n, graph=False, **kw)
    grids = [vm.Grid(extent, voxel) for _ in range(S)]
    moved = 0
    for k in range(frames):
        cloud = np.stack([rooms[s][0][k] for s in range(S)])
        init = np.stack([model.perturbed(rooms[s][1][k], 1.0, 0.1) if k else np.eye(4) for s in range(S)])
        T, steps = ref.register(_dev(cloud, cuda), _dev(init, cuda), trace=True)
        T = T.cpu().numpy()
        for s, g in enumerate(grids):
            status = 0
            for it, st in enumerate(steps):
                Tb = st["T_before"][s].cpu().numpy()
                row, mag, near = g.accumulate(cloud[s], Tb, 0.5, voxel)
                got = st["sum"][s].cpu().numpy()
                assert np.array_equal(st["cell"][s].cpu().numpy(), near[0]) and got[model.PAIRS] == row[model.PAIRS]
                assert np.array_equal(st["dist"][s].cpu().numpy().view(np.int32), near[2].view(np.int32))
                assert (np.abs(got - row) <= 1e-12 * mag + 1e-300).all(), (k, s, it)
                want = model.solve(got, Tb, status, it, 1e-6, 1e-4, 32)
                status = want["status"]
                assert int(st["status"][s]) == status, (k, s, it)
                assert np.abs(st["delta"][s].cpu().numpy() - want["delta"]).max() <= 1e-10
                assert np.abs(st["T"][s].cpu().numpy() - want["T"]).max() <= 1e-10
                moved += int(np.abs(want["delta"]).max() > 0)
            if k == 0:
                assert status == model.FEW_PAIRS and np.array_equal(T[s], init[s])
            g.push(cloud[s], ref.bufs["stage_normals"][s].cpu().numpy(), T[s])
            assert _grid_is(voxel_map.sections(ref.bufs["grid"], S, extent), s, g), (k, s)
            assert np.array_equal(ref.pose()[s].cpu().numpy(), g.P) and int(ref.bufs["seq"][s]) == g.seq == k + 1
    assert moved >= 2 * S
    _lib.synchronize(cuda)


# ---- 4. the whole refiner ----------------------------------------------------------------------------------------------------------

def test_refiner_on_the_box_room(cuda):
    S, n, frames = 2, 1024, 3
    kw = dict(voxel_size=1.0, extent=(16, 16, 8))
    rooms = [model.room(3 + s, frames, n) for s in range(S)]
    eager = voxel_map.VoxelMapRefiner(S, n, graph=False, **kw)
    graphed = voxel_map.VoxelMapRefiner(S, n, graph=True, **kw)
    again = voxel_map.VoxelMapRefiner(S, n, graph=True, **kw)
    grids = [vm.Grid(kw["extent"], 1.0) for _ in range(S)]
    graphs = set()
    for k in range(frames):
        cloud = np.stack([rooms[s][0][k] for s in range(S)])
        gt = np.stack([rooms[s][1][k] for s in range(S)])
        init = np.stack([model.perturbed(gt[s]) if k else np.eye(4) for s in range(S)])
        c, i = _dev(cloud, cuda), _dev(init, cuda)
        T = eager.register(c, i).clone()
        for ref in (graphed, again):
            assert _same(ref.register(c, i), T), k                  # eager = replay = a second run
            assert torch.equal(ref.bufs["grid"], eager.bufs["grid"]) and _same(ref.pose(), eager.pose())
        graphs.add(id(graphed._graph))
        for s in range(S):
            Tm, _, _ = vm.register(grids[s], cloud[s], init[s])     # the fp64 model, on its own normals and its own poses
            if k:
                dev_err, mod_err = model.pose_error(T[s].cpu().numpy(), gt[s]), model.pose_error(Tm, gt[s])
                print("frame %d stream %d: device %.3e model %.3e ratio %.3f guess %.3e"
                      % (k, s, dev_err, mod_err, dev_err / mod_err, model.pose_error(init[s], gt[s])))
                assert dev_err <= 1.5 * mod_err and dev_err < model.pose_error(init[s], gt[s])
    assert len(graphs) == 2 and graphed._graph is not None          # no graph, then one capture for good
    assert eager.map_bytes() == S * 16 * 16 * 8 * 264 == eager.bufs["grid"].numel()
    mp = eager.map_points(1)
    assert mp["points"].shape[0] == mp["normals"].shape[0] == mp["voxels"].shape[0] == mp["keys"].shape[0] > 500
    assert eager.bufs["seq"].tolist() == [frames] * S and eager.bufs["nonempty"].tolist() == [[1]] * S
    _lib.synchronize(cuda)


def test_launches_of_one_register(cuda):
    clouds, gt = model.room(3, 2, 256)
    counts = []
    for keyframe in (None, dict(trans=0.1, rot=0.3)):
        ref = voxel_map.VoxelMapRefiner(1, 256, extent=(16, 16, 8), iters=3, graph=False, keyframe=keyframe)
        ref.register(_dev(clouds[0][None], cuda), _dev(np.eye(4)[None], cuda))
        calls, real = [], _lib.call
        _lib.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
        try:
            ref.register(_dev(clouds[1][None], cuda), _dev(gt[1][None], cuda))
        finally:
            _lib.call = real
        counts.append([c for c in calls if c.endswith("kernel_wrapper")])
    assert counts[0] == ["voxel_begin_kernel_wrapper", "knn_build_kernel_wrapper", "knn_point_prebuilt_kernel_wrapper",
                         "icp_normals_kernel_wrapper"] + ["voxel_accumulate_kernel_wrapper",
                                                          "icp_solve_masked_kernel_wrapper"] * 3 + \
        ["voxel_insert_kernel_wrapper", "voxel_pose_kernel_wrapper"]
    assert counts[1] == counts[0][:-2] + ["keyframe_gate_kernel_wrapper"] + counts[0][-2:]
    _lib.synchronize(cuda)


# ---- 5. masks ----------------------------------------------------------------------------------------------------------------------

def test_per_stream_refiner_equals_lock_step_refiners_of_the_streams_own(cuda):
    S, n = masked.S, masked.N
    kw = dict(voxel_size=1.0, extent=(16, 16, 8), iters=6)
    multi = voxel_map.VoxelMapRefiner(S, n, graph=True, per_stream=True, **kw)
    singles = [voxel_map.VoxelMapRefiner(1, n, graph=False, **kw) for _ in range(S)]
    keys = ("P", "nonempty", "seq", "T", "status", "iterations", "pairs", "cost")
    graphs = set()
    for c, call in enumerate(masked.schedule()):
        if call["reset"]:
            multi.reset(streams=call["reset"])
            assert multi.bufs["armed"].tolist() == [int(s in call["reset"]) for s in range(S)]
        cloud, init = _dev(call["cloud"], cuda), _dev(call["init"], cuda)
        before = None if multi.bufs is None else {k: multi.bufs[k].clone() for k in keys + ("grid",)}
        T = multi.register(cloud, init, active=call["active"].tolist(), restart=_dev(call["restart"], cuda))
        if multi._graph is not None:
            graphs.add(id(multi._graph))
        sec = voxel_map.sections(multi.bufs["grid"], S, kw["extent"])
        was = None if before is None else voxel_map.sections(before["grid"], S, kw["extent"])
        for s in range(S):
            if not call["active"][s]:
                assert _same(T[s], init[s]) and int(multi.status()[s]) == masked.IDLE
                assert int(multi.diagnostics()["iterations"][s]) == 0 and int(multi.diagnostics()["pairs"][s]) == 0
                if before is not None:
                    for k in ("P", "nonempty", "seq"):
                        assert _same(multi.bufs[k][s], before[k][s]), (c, s, k)
                    for k in sec:
                        assert _same(sec[k][s], was[k][s]), (c, s, k)
                continue
            if call["primes"][s]:
                singles[s].reset()
            singles[s].register(cloud[s:s + 1].contiguous(), init[s:s + 1].contiguous())
            for k in keys:
                assert _same(multi.bufs[k][s], singles[s].bufs[k][0]), (c, s, k)
            one = voxel_map.sections(singles[s].bufs["grid"], 1, kw["extent"])
            for k in sec:
                assert _same(sec[k][s], one[k][0]), (c, s, k)
            if call["primes"][s]:                                   # begin: restart and armed words alike
                assert int(multi.status()[s]) == model.FEW_PAIRS and _same(T[s], init[s])
                assert int(multi.bufs["seq"][s]) == 1 and int(multi.bufs["nonempty"][s, 0]) == 1
                assert _same(multi.pose()[s], torch.eye(4, dtype=torch.float64, device=cuda))
                assert int((multi.map_points(s)["keys"] >> 32).max()) == 0       # only this frame is in the map
            else:
                assert not int(multi.status()[s]) & (model.FEW_PAIRS | model.BAD_PIVOT | masked.IDLE), (c, s)
        assert multi.bufs["armed"].tolist() == [0] * S or not all(call["active"])
    assert len(graphs) == 1 and multi.calls == masked.CALLS         # one capture
    _lib.synchronize(cuda)


# ---- 6. keyframes ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _walk(n):
    data = [kf.room_walk(3 + s, kf.steps(kf.WALK[s]), n) for s in range(2)]
    clouds, gt = np.stack([d[0] for d in data], axis=1), np.stack([d[1] for d in data], axis=1)
    init = np.stack([[model.perturbed(gt[k, s]) if k else np.eye(4) for s in range(2)] for k in range(gt.shape[0])])
    return clouds, gt, init


def test_refiner_with_keyframes(cuda):
    S, n = 2, 1024
    clouds, gt, init = _walk(n)
    kw = dict(voxel_size=1.0, extent=(16, 16, 8), iters=6)
    keyed = voxel_map.VoxelMapRefiner(S, n, graph=True, keyframe=kf.WALK_KEYFRAME, **kw)
    every = voxel_map.VoxelMapRefiner(S, n, graph=True, keyframe=dict(trans=0.0, rot=0.0), **kw)
    none = voxel_map.VoxelMapRefiner(S, n, graph=True, **kw)
    assert keyed.keyframe_state() is None and none.keyframe_state() is None
    gates = [kf.Gate(**kf.WALK_KEYFRAME) for _ in range(S)]
    for k in range(clouds.shape[0]):
        c, i = _dev(clouds[k], cuda), _dev(init[k], cuda)
        live = keyed.bufs["nonempty"][:, 0].tolist() if keyed.bufs is not None else [0] * S
        pose_before = None if keyed.bufs is None else keyed.pose().cpu().numpy().copy()
        T = keyed.register(c, i).cpu().numpy()
        state = keyed.keyframe_state()
        for s, g in enumerate(gates):
            assert g.margin(T[s], bool(live[s])) > 1e-9
            g.step(T[s], bool(live[s]))
            assert int(state["insert"][s]) == g.insert == kf.WALK_INSERTS[k] and int(state["count"][s]) == g.count, (k, s)
            assert np.abs(state["delta"][s].cpu().numpy() - g.delta).max() <= 1e-12
            if k:                                                   # inserted or not, the pose follows the frame
                assert np.array_equal(keyed.pose()[s].cpu().numpy(), vm.pose_mul(pose_before[s], T[s]))
                assert model.pose_error(T[s], gt[k, s]) <= 0.5 * model.pose_error(init[k, s], gt[k, s])
        assert keyed.bufs["seq"].tolist() == [sum(kf.WALK_INSERTS[:k + 1])] * S
        a, b = every.register(c, i), none.register(c, i)            # thresholds every frame exceeds
        assert _same(a, b) and every.keyframe_state()["insert"].tolist() == [1] * S
        for x, y in ((every.status(), none.status()), *zip(every.diagnostics().values(), none.diagnostics().values()),
                     *zip(every.map_state().values(), none.map_state().values()), (every.bufs["grid"], none.bufs["grid"])):
            assert _same(x, y), k
        assert every.keyframe_state()["count"].tolist() == [k + 1] * S
    assert sorted(none.bufs) == sorted(set(every.bufs) - {"kf_delta", "kf_insert", "kf_count"})
    assert keyed.keyframe_state()["count"].tolist() == [4] * S
    _lib.synchronize(cuda)


def test_a_standing_sensor_inserts_once(cuda):
    n = 1024
    cloud = _dev(model.room(3, 1, n)[0], cuda)
    eye = torch.eye(4, dtype=torch.float64, device=cuda)[None].contiguous()
    ref = voxel_map.VoxelMapRefiner(1, n, extent=(16, 16, 8), iters=3, keyframe=dict(trans=10.0, rot=90.0))
    stored = None
    for k in range(4):
        ref.register(cloud, eye)
        assert ref.keyframe_state()["insert"].tolist() == [int(k == 0)] and ref.bufs["seq"].tolist() == [1]
        stored = ref.bufs["grid"].clone() if stored is None else stored
        assert torch.equal(ref.bufs["grid"], stored)
    assert ref.keyframe_state()["count"].tolist() == [1]
    _lib.synchronize(cuda)
