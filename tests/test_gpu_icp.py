"""Point-to-plane registration on the device against the NumPy fp64 model of tests/icp_model.py:
the ops alone (normals, queries, accumulate with planted inputs, solve), a whole registration teacher-forced iteration by
iteration, graph replay against eager, the result against ground truth and against the model's own result, the sliding
map's bookkeeping, and ``StreamingOdometry(refine=...)``.

Bounds.  Normals: 1 - |n . n_model| <= 64 eps64 / gap for points with relative eigen-gap >= 1e-3 (fp64 rounding times the
eigenvector's conditioning).  The kernel's output is fp32, whose length is off 1 by up to 2^-24 sqrt(3): n is compared as
a direction (normalised in fp64), and its length is checked on its own; rounding to fp32 turns a direction by at most
2^-24 sqrt(3), 1.4e-15 in this measure, a tenth of the bound at gap = 1.  Sums: 1e-12 of the sum of the terms' magnitudes.
Steps and poses: 1e-10, norm-wise relative.  Ground truth: 1.5 times the model's error plus 1e-5, and a tenth of the
initial guess's error."""
import functools

import numpy as np
import pytest
import torch

import icp_model as model
from oracle import params
from pwclonet_pylidarslam_amd import _lib, registration, synthetic
from pwclonet_pylidarslam_amd.odometry import StreamingOdometry
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet

pytestmark = pytest.mark.gpu


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    """Two device tensors hold the same bits (floating tensors compared as integers)."""
    raw = lambda t: t.contiguous().view({8: torch.int64, 4: torch.int32}[t.element_size()]) if t.dtype.is_floating_point else t
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(raw(a), raw(b))


def _ulps(a, b):
    """Distance in fp32 steps between finite arrays a and b (b fp64: first rounded to fp32)."""
    key = lambda x: np.where(_bits(x).view(np.int32) < 0, np.int64(-(2 ** 31)) - _bits(x).view(np.int32), _bits(x).view(np.int32)).astype(np.int64)
    return np.abs(key(a) - key(np.asarray(b).astype(np.float32)))


# ---- 1. normals ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("b, n, k", model.NORMAL_SHAPES)
def test_normals_against_the_model(cuda, b, n, k):
    x = model.normals_cloud(b, n)
    got, eig = registration.normals(_dev(x, cuda), k)
    got, eig = got.cpu().numpy(), eig.cpu().numpy()
    for c in range(b):
        want, val, gap = model.normals(x[c], k)
        use = gap >= model.GAP_MIN
        assert (~use).mean() <= model.GAP_CAP
        g = got[c].astype(np.float64)
        length = np.linalg.norm(g, axis=1)
        assert (np.abs(length - 1.0) <= 2.0 ** -23).all()
        miss = 1.0 - np.abs(np.einsum("ni,ni->n", g / length[:, None], want))
        ratio = miss[use] / (64.0 * model.EPS64 / gap[use])
        print("normals b=%d n=%d k=%d cloud %d: worst miss / bound = %.3g, left out %d" % (b, n, k, c, ratio.max(), (~use).sum()))
        assert (ratio <= 1.0).all()
        assert (np.einsum("ni,ni->n", g, x[c].astype(np.float64)) <= 0.0).all()          # towards the origin
        assert np.abs(eig[c] - val).max() <= 64.0 * model.EPS64 * val[:, 2].max()
        assert (np.diff(eig[c], axis=1) >= 0.0).all()
    _lib.synchronize(cuda)


def test_degenerate_neighbourhoods_give_zero_normals(cuda):
    line = np.zeros((65, 3), dtype=np.float32)
    line[:, 0] = np.arange(65) * 0.5 + 1.0
    diag = np.repeat((np.arange(65, dtype=np.float32) * 0.25 + 2.0)[:, None], 3, axis=1)
    dup = np.tile(np.array([[1.0, 2.0, 3.0]], dtype=np.float32), (65, 1))
    mixed = model.normals_cloud(1, 65)[0]
    mixed[:12] = mixed[0]                                                      # 12 copies: their 10 neighbours are copies
    x = np.stack([line, diag, dup, mixed])
    got, eig = registration.normals(_dev(x, cuda), 10)
    got = got.cpu().numpy()
    assert not got[:3].any()
    want = model.normals(mixed, 10)[0]                       # a point whose 10 nearest are the copies is degenerate too
    assert not got[3, :12].any() and not want[:12].any() and want[12:].any(axis=1).sum() > 40
    assert np.array_equal(got[3].any(axis=1), want.any(axis=1))
    _lib.synchronize(cuda)


# ---- 2. queries ------------------------------------------------------------------------------------------------------------

def test_queries_within_one_ulp_and_exact_for_the_identity(cuda):
    r = np.random.default_rng(4)
    S, M, n = 2, 3, 1000
    p = r.uniform(-40.0, 40.0, (S, n, 3)).astype(np.float32)
    A = np.stack([np.stack([model.pose(model.rot(r.normal(size=3), r.uniform(0, 3)), r.normal(size=3) * 5) for _ in range(M)])
                  for _ in range(S)])
    T = np.stack([model.pose(model.rot(r.normal(size=3), 0.1), r.normal(size=3)) for _ in range(S)])
    for t in (None, T):
        got = registration.queries(_dev(A, cuda), _dev(p, cuda), None if t is None else _dev(t, cuda)).cpu().numpy()
        for s in range(S):
            want = model.queries(A[s], p[s], None if t is None else t[s])[0]
            assert _ulps(got[s], want).max() <= 1
    eye = np.tile(np.eye(4), (S, M, 1, 1))
    for t in (None, eye[:, 0]):
        got = registration.queries(_dev(eye, cuda), _dev(p, cuda), None if t is None else _dev(t, cuda)).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(np.repeat(p[:, None], M, axis=1)))
    _lib.synchronize(cuda)


# ---- 3. accumulate with planted inputs -------------------------------------------------------------------------------------

def _accumulate(c, dev):
    t = {k: _dev(v, dev) for k, v in c.items() if isinstance(v, np.ndarray)}
    return registration.accumulate(t["p"], t["q"], t["idx"], t["dist"], t["map_xyz"], t["map_normals"], t["live"], t["R"],
                                   t["T"], c["sigma"], c["max_dist"])


def test_accumulate_planted_inputs(cuda):
    c = model.planted()
    S, n = c["p"].shape[:2]
    a, b = _accumulate(c, cuda), _accumulate(c, cuda)
    assert a.shape == (S, registration.groups(n), 32) and registration.groups(n) == 2
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))                # two runs: the same bits
    got = a.cpu().numpy()
    assert np.isfinite(got).all() and not got[:, :, 30:].any()                  # the dead slot's NaNs were not read
    for s in range(S):
        want, mag = model.accumulate(c["p"][s], c["q"][s], c["idx"][s], c["dist"][s], c["map_xyz"][s], c["map_normals"][s],
                                     c["live"][s], c["R"][s], c["T"][s], c["sigma"], c["max_dist"])
        err = np.abs(got[s].sum(axis=0) - want)
        print("accumulate stream %d: pairs %d, worst err / (1e-12 sum|term|) = %.3g"
              % (s, want[model.PAIRS], (err / np.maximum(1e-12 * mag, 1e-300))[mag > 0].max() if (mag > 0).any() else 0.0))
        assert (err <= 1e-12 * mag).all()
        assert got[s].sum(axis=0)[model.PAIRS] == want[model.PAIRS]
    assert not got[2].any()                                                     # every point rejected: exact zeros
    _lib.synchronize(cuda)


# ---- 4. solve --------------------------------------------------------------------------------------------------------------

def _solve(rows, T, status, dev, it=0, **kw):
    """rows (S, 32) presented as two partial rows per stream (a split that adds back exactly)."""
    half = np.ldexp(rows, -1)
    partial = np.stack([half, rows - half], axis=1)
    Td, sd = _dev(T, dev), _dev(np.asarray(status, dtype=np.int32), dev)
    out = registration.solve(_dev(partial, dev), Td, sd, it=it, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}, Td.cpu().numpy(), sd.cpu().numpy()


def _close(got, want, what):
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    print("%s: err / (1e-10 scale) = %.3g" % (what, err / (1e-10 * scale) if scale > 0 else err))
    assert err <= 1e-10 * scale, what


def test_solve_against_the_model(cuda):
    r = np.random.default_rng(6)
    T0 = np.stack([model.pose(model.rot(r.normal(size=3), 0.4), r.normal(size=3)) for _ in range(3)])
    rows = np.stack([model.planted_rows(seed=23), model.planted_rows(seed=24, flat=True), model.planted_rows(seed=25)])
    kw = dict(damping=1e-6, threshold_delta_pose=1e-4, min_pairs=64)
    out, T, st = _solve(rows, T0, [7, 7, 7], cuda, **kw)                        # it = 0 clears stale status words
    for s in range(3):
        want = model.solve(rows[s], T0[s], 7, 0, 1e-6, 1e-4, 64)
        _close(out["delta"][s], want["delta"], "delta %d" % s)
        _close(T[s], want["T"], "T %d" % s)
        assert st[s] == want["status"] == 0 and out["iterations"][s] == 1 and out["pairs"][s] == int(rows[s][model.PAIRS])
        assert out["cost"][s] == rows[s][model.COST] and np.array_equal(out["sum"][s], rows[s])
        assert np.abs(T[s][:3, :3] @ T[s][:3, :3].T - np.eye(3)).max() < 1e-14 and T[s][3].tolist() == [0, 0, 0, 1]
    assert out["delta"][1][5] == 0.0                                            # the null direction: a zero step
    # a tiny step sets the converged bit and is still applied
    tiny = rows[0].copy()
    tiny[model.G0:model.G0 + 6] *= 1e-7
    out, T, st = _solve(tiny[None], T0[:1], [0], cuda, **kw)
    want = model.solve(tiny, T0[0], 0, 0, 1e-6, 1e-4, 64)
    assert st[0] == want["status"] == model.CONVERGED and not np.array_equal(T[0], T0[0])
    _close(T[0], want["T"], "T converged")
    _lib.synchronize(cuda)


def test_solve_freezes_and_leaves_the_pose_alone(cuda):
    r = np.random.default_rng(7)
    T0 = np.stack([model.pose(model.rot(r.normal(size=3), 0.4), r.normal(size=3)) for _ in range(3)])
    good = model.planted_rows(seed=23)
    # a pivot that is not positive (damping 0 on the exactly rank-deficient system), and too few pairs
    rows = np.stack([good, model.planted_rows(seed=24, flat=True), model.planted_rows(seed=26, pairs=10)])
    out, T, st = _solve(rows, T0, [0, 0, 0], cuda, damping=0.0, threshold_delta_pose=1e-4, min_pairs=64)
    assert st.tolist() == [0, model.BAD_PIVOT, model.FEW_PAIRS]
    assert np.array_equal(T[1:].view(np.int64), T0[1:].view(np.int64)) and not out["delta"][1:].any()
    assert not np.array_equal(T[0], T0[0])
    assert out["iterations"].tolist() == [1, 1, 1] and out["pairs"][2] == 10
    # the next iteration: the frozen streams stay bit for bit while stream 0 goes on
    rows2 = np.stack([model.planted_rows(seed=27), good, good])
    out2, T2, st2 = _solve(rows2, T, st, cuda, it=1, damping=0.0, threshold_delta_pose=1e-4, min_pairs=64)
    want = model.solve(rows2[0], T[0], 0, 1, 0.0, 1e-4, 64)
    _close(T2[0], want["T"], "T of the live stream")
    assert np.array_equal(T2[1:].view(np.int64), T0[1:].view(np.int64)) and not out2["delta"][1:].any()
    assert st2.tolist() == [0, model.BAD_PIVOT, model.FEW_PAIRS] and out2["iterations"][0] == 2
    _lib.synchronize(cuda)


# ---- 5. whole registrations ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _rooms(S, frames, n):
    data = [model.room(3 + s, frames, n) for s in range(S)]
    return np.stack([d[0] for d in data], axis=1), np.stack([d[1] for d in data], axis=1)      # (frames, S, ...)


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("M", [1, 3])
def test_registration_teacher_forced_and_graph_replay(cuda, M, S):
    n, frames = 1024, 4
    clouds, gt = _rooms(S, frames, n)
    kw = dict(map_size=M, iters=6)
    eager = registration.IcpRefiner(S, n, graph=False, **kw)
    graphed = registration.IcpRefiner(S, n, graph=True, **kw)
    for k in range(frames):
        init = np.stack([model.perturbed(gt[k, s]) if k else np.eye(4) for s in range(S)])
        before = None if eager.bufs is None else {key: v.cpu().numpy() for key, v in eager.bufs.items()
                                                  if key in ("map_xyz", "map_normals", "live", "A", "R")}
        T, steps = eager.register(_dev(clouds[k], cuda), _dev(init, cuda), trace=True)
        T = T.cpu().numpy().copy()
        Tg = graphed.register(_dev(clouds[k], cuda), _dev(init, cuda)).cpu().numpy()
        assert np.array_equal(T.view(np.int64), Tg.view(np.int64)), k          # replay (k >= 1) = eager, bit for bit
        if k == 0:                                                              # the first frame only fills the map
            assert np.array_equal(T, init) and eager.status().tolist() == [model.FEW_PAIRS] * S
            continue
        assert len(steps) == 6
        for s in range(S):
            status = 0
            for it, st in enumerate(steps):
                tb = st["T_before"][s].cpu().numpy()
                q, idx, dist = st["q"][s].cpu().numpy(), st["idx"][s].cpu().numpy(), st["dist"][s].cpu().numpy()
                assert _ulps(q, model.queries(before["A"][s], clouds[k, s], tb)[0]).max() <= 1
                mi, md = model.search(q, before["map_xyz"][s])
                live = before["live"][s] != 0
                assert np.array_equal(idx[live], mi[live]) and np.array_equal(_bits(dist[live]), _bits(md[live]))
                row, mag = model.accumulate(clouds[k, s], q, idx, dist, before["map_xyz"][s], before["map_normals"][s],
                                            before["live"][s], before["R"][s], tb, 0.5, 1.0)
                assert (np.abs(st["sum"][s].cpu().numpy() - row) <= 1e-12 * mag).all()
                want = model.solve(row, tb, status, it, 1e-6, 1e-4, 64)
                if want["delta"].any():
                    _close(st["delta"][s].cpu().numpy(), want["delta"], "frame %d stream %d iteration %d delta" % (k, s, it))
                else:                                                           # frozen: no step at all
                    assert not st["delta"][s].cpu().numpy().any()
                _close(st["T"][s].cpu().numpy(), want["T"], "T")
                status = want["status"]
                assert int(st["status"][s]) == status
            assert model.pose_error(T[s], gt[k, s]) <= 0.1 * model.pose_error(init[s], gt[k, s])
    assert graphed._graph is not None and graphed.calls == frames
    _lib.synchronize(cuda)


def test_against_ground_truth_and_the_models_own_result(cuda):
    S, M, n, frames = 2, 3, 1024, 4
    clouds, gt = _rooms(S, frames, n)
    ref = registration.IcpRefiner(S, n, map_size=M, graph=True)
    maps = [model.Map(M, n, 10) for _ in range(S)]
    worst = 0.0
    for k in range(frames):
        init = np.stack([model.perturbed(gt[k, s]) if k else np.eye(4) for s in range(S)])
        T = ref.register(_dev(clouds[k], cuda), _dev(init, cuda)).cpu().numpy()
        for s in range(S):
            Tm, _, _ = model.register(maps[s], clouds[k, s], init[s])
            if k == 0:
                continue
            e0, em, ed = (model.pose_error(x, gt[k, s]) for x in (init[s], Tm, T[s]))
            worst = max(worst, ed / em)
            print("frame %d stream %d: init %.4g, model %.4g, device %.4g, device / model %.4f" % (k, s, e0, em, ed, ed / em))
            assert ed <= 1.5 * em + 1e-5
            assert ed <= 0.1 * e0
        if k:
            assert not (ref.status().cpu().numpy() & (model.FEW_PAIRS | model.BAD_PIVOT)).any()
            d = ref.diagnostics()
            assert (d["pairs"].cpu().numpy() > 0.9 * n).all() and (d["iterations"].cpu().numpy() >= 1).all()
    print("worst device / model error ratio %.4f" % worst)
    _lib.synchronize(cuda)


# ---- 6. the map ------------------------------------------------------------------------------------------------------------

def test_map_bookkeeping_and_partial_reset(cuda):
    S, M, n = 2, 2, 256
    frames = M + 2
    clouds, gt = _rooms(S, frames, n)
    ref = registration.IcpRefiner(S, n, map_size=M, iters=2, graph=False)
    twin = registration.IcpRefiner(S, n, map_size=M, iters=2, graph=False)      # the same frames, never reset
    maps = [model.Map(M, n, 10) for _ in range(S)]
    for k in range(frames):
        twin.register(_dev(clouds[k], cuda), _dev(gt[k], cuda))
        T = ref.register(_dev(clouds[k], cuda), _dev(gt[k], cuda)).cpu().numpy().copy()
        state = {key: v.cpu().numpy() for key, v in ref.map_state().items()}
        nrm = ref.bufs["stage_normals"].cpu().numpy()
        for s in range(S):
            maps[s].push(clouds[k, s], T[s], nrm[s])                            # the model's push with the device's pose
            assert state["live"][s].tolist() == maps[s].live.tolist() and state["cursor"][s] == maps[s].cursor
            assert np.abs(state["A"][s] - maps[s].A).max() <= 1e-13 and np.abs(state["R"][s] - maps[s].R).max() <= 1e-13
            assert np.array_equal(ref.bufs["map_xyz"][s].cpu().numpy(), maps[s].xyz)
            assert np.array_equal(ref.bufs["map_normals"][s].cpu().numpy(), maps[s].normals)
    assert state["live"].tolist() == [[1, 1], [1, 1]]
    keep = {key: v.clone() for key, v in ref.map_state().items()}
    ref.reset(streams=[1])
    now = ref.map_state()
    for key in keep:                                                            # armed only: the old maps until a frame comes
        assert _same_bits(now[key], keep[key]), key
    assert ref.bufs["armed"].tolist() == [0, 1]
    init = np.stack([gt[1, 0], model.perturbed(gt[1, 1])])
    twin.register(_dev(clouds[1], cuda), _dev(init, cuda))
    T = ref.register(_dev(clouds[1], cuda), _dev(init, cuda)).cpu().numpy()
    assert np.array_equal(T[1], init[1]) and ref.status().tolist()[1] == model.FEW_PAIRS    # stream 1 only fills its map
    now = ref.map_state()
    assert now["live"].tolist() == [[1, 1], [1, 0]] and int(now["cursor"][1]) == 1 and ref.bufs["armed"].tolist() == [0, 0]
    assert torch.equal(now["A"][1, 0], torch.eye(4, dtype=torch.float64, device=cuda))
    for key in ("T", "status", "iterations", "pairs", "cost", "A", "R", "live", "cursor", "map_xyz", "map_normals"):
        assert _same_bits(ref.bufs[key][0], twin.bufs[key][0]), key             # stream 0: as if nothing had been reset
    _lib.synchronize(cuda)


# ---- 6b. lock step is a view of the masked engine --------------------------------------------------------------------------

@pytest.mark.parametrize("graph", [False, True])
def test_lock_step_and_per_stream_views_run_one_engine(cuda, graph):
    """A lock-step refiner and a per-stream refiner called without masks hold the same bits after every call, allocate the
    same buffers, and from the second call on no launch writes the mask words (their version counters stand still)."""
    S, M, n, frames = 2, 2, 256, 4
    clouds, gt = _rooms(S, frames, n)
    lock = registration.IcpRefiner(S, n, map_size=M, iters=2, graph=graph)
    per = registration.IcpRefiner(S, n, map_size=M, iters=2, graph=graph, per_stream=True)
    # not map_ws: the build orders the points of a cell by an atomic counter, so a structure's bytes vary from run to run
    keys = ("T", "status", "iterations", "pairs", "cost", "A", "R", "live", "cursor", "map_xyz", "map_normals")
    versions = None
    for k in range(frames):
        init = _dev(np.stack([model.perturbed(gt[k, s]) if k else np.eye(4) for s in range(S)]), cuda)
        Tl = lock.register(_dev(clouds[k], cuda), init)
        Tp = per.register(_dev(clouds[k], cuda), init, active=None, restart=None)
        assert _same_bits(Tl, Tp), k
        assert sorted(lock.bufs) == sorted(per.bufs)
        for key in keys:
            assert _same_bits(lock.bufs[key], per.bufs[key]), (k, key)
        for ref in (lock, per):
            assert ref.bufs["active"].tolist() == [1] * S and ref.bufs["restart"].tolist() == [0] * S
        now = [ref.bufs[w]._version for ref in (lock, per) for w in ("active", "restart")]
        assert versions is None or now == versions, k
        versions = now
    assert lock.status().tolist() == per.status().tolist() and not (lock.status().cpu().numpy() & model.FEW_PAIRS).any()
    assert (lock._graph is not None) == (per._graph is not None) == graph
    _lib.synchronize(cuda)


# ---- 7. streaming odometry -------------------------------------------------------------------------------------------------

def _net(dev):
    """The suite's synthetic weights, with the last layer of every pose head set to (q, t) = ((1, 0, 0, 0), 0): the
    untrained network's pose is no motion at all (DESIGN.md section 20 measured 1.9 m and ~126 degrees), and no
    registration starts from that; this one estimates "no motion", a guess 0.5-1.5 m and up to 2 degrees off."""
    net = PWCLONet(dict(num_input_channels=3, sequence_len=2, device=str(dev), scalar_last=False, log_mode="none",
                        fused="auto"))
    sd = net.state_dict()
    params.fill_state_dict(sd)
    heads = 0
    for key, v in sd.items():
        if key.endswith(("conv1d_q.conv.weight", "conv1d_t.conv.weight", "conv1d_t.conv.bias")):
            v.zero_()
        elif key.endswith("conv1d_q.conv.bias"):
            v.copy_(torch.tensor([1.0, 0.0, 0.0, 0.0]))
            heads += 1
    assert heads == 4
    net = net.to(dev).eval()
    net.prepare_fused()
    return net


def test_streaming_odometry_with_refine(cuda):
    """Walls only (synthetic drops the ground): the vertical (camera y) is constrained by the noise of the normals alone.
    The device's vertical correction must stay within the model's on the same clouds and initial guesses, with the margin
    of the ground-truth test."""
    S, n, frames, iters = 2, 1024, 4, 8
    seq = torch.from_numpy(np.stack([synthetic.kitti_like_sequence(31 + i, n, frames)[0] for i in range(S)], axis=1)).to(cuda)
    net = _net(cuda)
    cfg = dict(map_size=2, iters=iters, max_dist=2.0)
    plain = StreamingOdometry(net, streams=S, graph=True)
    refined = StreamingOdometry(net, streams=S, graph=True, refine=cfg)
    with torch.no_grad():
        for k in range(frames):
            a, b = plain.step(seq[k]), refined.step(seq[k])
            assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
            if k:
                st = refined.refiner().status().cpu().numpy()
                print("frame %d status %s pairs %s" % (k, st.tolist(), refined.refiner().diagnostics()["pairs"].tolist()))
                assert not (st & (model.FEW_PAIRS | model.BAD_PIVOT)).any()
    assert torch.equal(plain.relative_poses(), refined.relative_poses())
    assert torch.equal(plain.trajectory(), refined.trajectory())
    rel, ref = refined.relative_poses().cpu().numpy(), refined.refined_relative_poses().cpu().numpy()
    assert np.abs(rel - np.eye(4)).max() < 1e-6                                 # the guess: no motion
    assert ref.shape == rel.shape == (frames, S, 4, 4) and np.array_equal(ref[0], rel[0])
    traj = refined.refined_trajectory().cpu().numpy()
    host = seq[:, :, :, :3].cpu().numpy()
    for s in range(S):
        mp = model.Map(2, n, 10)
        acc = np.eye(4)
        for k in range(frames):
            Tm, _, _ = model.register(mp, host[k, s], rel[k, s], iters=iters, max_dist=2.0)
            acc = acc @ ref[k, s]
            assert np.abs(traj[k, s] - acc).max() <= 1e-12 * max(1.0, np.abs(acc).max())
            if k:
                dy_dev, dy_model = abs(ref[k, s, 1, 3] - rel[k, s, 1, 3]), abs(Tm[1, 3] - rel[k, s, 1, 3])
                print("frame %d stream %d: vertical correction device %.4g model %.4g" % (k, s, dy_dev, dy_model))
                assert dy_dev <= 1.5 * dy_model + 1e-5
                assert np.linalg.norm(ref[k, s, :3, 3]) > 0.3                   # and the registration found the motion
    with pytest.raises(ValueError, match="per_stream"):
        StreamingOdometry(net, streams=S, per_stream=True, refine=cfg)
    graph = refined.refiner()._graph
    refined.reset()                                                             # a new sequence: the maps start over too
    assert refined.refiner().bufs["armed"].tolist() == [1] * S
    with torch.no_grad():
        assert refined.step(seq[2]) is None and refined.refiner().status().tolist() == [model.FEW_PAIRS] * S
        assert refined.step(seq[3]) is not None
    again = refined.refined_relative_poses()
    assert again.shape == (2, S, 4, 4) and _same_bits(again[0], torch.eye(4, dtype=torch.float64, device=cuda).expand(S, 4, 4))
    assert np.linalg.norm(again[1, :, :3, 3].cpu().numpy(), axis=1).min() > 0.3
    assert refined.captures == 1 and graph is not None and refined.refiner()._graph is graph    # one graph each, all along
    assert refined.refiner().calls == frames + 2
    _lib.synchronize(cuda)
