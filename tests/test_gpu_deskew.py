"""Motion compensation of raw sweeps on the device: the stand-alone op against the NumPy model of
tests/deskew_model.py (correct rounding of a value within fp64 noise of the model; bit for bit where the rule says so), the
raw front end against the chain of ops, streaming odometry in lock step and per stream against that chain with the motions
the rule prescribes, and the unchanged default.  Everything but the op-against-model bound is compared exactly."""
import functools

import numpy as np
import pytest
import torch

import deskew_model as model
from oracle import params
from pwclonet_pylidarslam_amd import _lib, preprocess, synthetic
from pwclonet_pylidarslam_amd.odometry import StreamingOdometry
from pwclonet_pylidarslam_amd.pointnet2_ops import _ext
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet

pytestmark = pytest.mark.gpu

NEAR = 30.0
VELO_TO_CAM = np.array([[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0], [1.0, 0.0, 0.0, 0.0]])
NAMES = list(model.MOTIONS) + ["identity"]
ROWS = np.stack(list(model.MOTIONS.values()) + [model.IDENTITY])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. the stand-alone op against the model -------------------------------------------------------------------------------

def _points(b, n, stride, seed):
    r = np.random.default_rng([seed, b, n])
    pts = (r.random((b, n, stride)) * 160.0 - 80.0).astype(np.float32)
    pts[..., 2] = pts[..., 2] / 20.0
    return pts


def _sweep_times(b, n, seed, dtype):
    """Scan order with jitter: fp64 at an epoch time (0.1 s per sweep), fp32 from zero (an epoch does not fit fp32)."""
    r = np.random.default_rng([seed, 77, n])
    frac = np.sort(r.random((b, n)), axis=1)
    return (1.6e9 + 0.1 * frac) if dtype == np.float64 else (0.1 * frac).astype(np.float32)


def _op(points, times, rows, lengths=None, keep=None, dev=None):
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=dev)
    kp = None if keep is None else torch.from_numpy(keep).to(dev)
    out = preprocess.deskew(torch.from_numpy(points).to(dev), torch.from_numpy(times).to(dev),
                            torch.from_numpy(rows).to(dev), lengths=ln, keep=kp)
    return out.cpu().numpy()


def _assert_within_the_bound(got, points, times, rows, names, keep=None, lengths=None):
    m, want = model.deskew_batch(points, times, rows, keep, lengths)
    err, tol = np.abs(got.astype(np.float64) - m), model.bound(m, points, rows)
    for c, name in enumerate(names):
        alpha, cand = model.alphas(times[c], None if keep is None else keep[c], None if lengths is None else lengths[c])
        assert (err[c] <= tol[c]).all(), (name, float((err[c] / tol[c]).max()), int(np.argmax((err[c] / tol[c]).max(axis=1))))
        still = ~cand | (alpha == 0.0)                                       # bit for bit: alpha = 0 and non-candidates
        assert np.array_equal(_bits(got[c][still]), _bits(points[c][still, :3])), name
        if name in ("identity",):
            assert np.array_equal(_bits(got[c]), _bits(points[c][:, :3]))
    return m, want


@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1025, 5000])
def test_op_against_the_model(cuda, n, stride):
    b = len(NAMES)                                                            # one launch: a cloud per motion
    points, times = _points(b, n, stride, 1), _sweep_times(b, n, 2, np.float64)
    got = _op(points, times, ROWS, dev=cuda)
    m, want = _assert_within_the_bound(got, points, times, ROWS, NAMES)
    if n >= 1023:
        moved = [float(np.abs(m[c] - points[c][:, :3]).max()) for c in range(b)]
        assert min(moved[:-1]) > 0.1 and moved[-1] == 0.0                     # the inputs do what their names say
        assert (got == want).mean() > 0.99                                    # and device and libm agree nearly everywhere
    _lib.synchronize(cuda)


@pytest.mark.parametrize("tdtype", [np.float32, np.float64], ids=["t32", "t64"])
@pytest.mark.parametrize("with_keep", [False, True], ids=["all", "keep"])
@pytest.mark.parametrize("stride", [3, 4])
def test_three_clouds_of_different_lengths(cuda, stride, with_keep, tdtype):
    n, lengths, names = 3000, [3000, 1, 1777], ["2deg", "w<0", "179deg"]
    rows = np.stack([model.MOTIONS[k] for k in names])
    points, times = _points(3, n, stride, 5), _sweep_times(3, n, 6, tdtype)
    keep = None
    if with_keep:
        keep = (np.random.default_rng(8).random((3, n)) < 0.6).astype(np.int32)
        keep[1, 0] = 1
        big = np.finfo(tdtype).max
        times[keep == 0] = np.resize(np.array([np.nan, big, -big, np.inf], dtype=tdtype), int((keep == 0).sum()))
    for c, ln in enumerate(lengths):                                          # rows past a length: anything at all
        times[c, ln:] = np.resize(np.array([-np.inf, np.nan, 1e30, -1e30], dtype=tdtype), n - ln)
    got = _op(points, times, rows, lengths=lengths, keep=keep, dev=cuda)
    m, _ = _assert_within_the_bound(got, points, times, rows, names, keep, lengths)
    assert np.array_equal(_bits(got[1]), _bits(points[1][:, :3]))             # one candidate: no time range, nobody moves
    for c in (0, 2):
        assert np.abs(m[c] - points[c][:, :3]).max() > 0.1 and np.isfinite(m[c]).all()
        assert np.array_equal(_bits(got[c, lengths[c]:]), _bits(points[c, lengths[c]:, :3]))
    _lib.synchronize(cuda)


def test_a_kept_row_without_a_finite_time_keeps_its_bits(cuda):
    n = 2000
    points, times = _points(2, n, 3, 9), _sweep_times(2, n, 10, np.float64)
    times[0, [0, 7, 1999]] = [np.nan, np.inf, -np.inf]
    times[1] = np.nan                                                         # no finite time at all
    rows = np.stack([model.MOTIONS["90deg"]] * 2)
    got = _op(points, times, rows, dev=cuda)
    _assert_within_the_bound(got, points, times, rows, ["90deg", "no times"])
    assert np.array_equal(_bits(got[0, [0, 7, 1999]]), _bits(points[0, [0, 7, 1999]]))
    assert np.array_equal(_bits(got[1]), _bits(points[1])) and (got[0] != points[0]).any()
    _lib.synchronize(cuda)


# ---- 2. the raw front end = the chain of ops -------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _sweeps(seed, frames, n_azimuth):
    return synthetic.raw_sweep_sequence(seed, frames, n_azimuth=n_azimuth)[0]


def _trs(S):
    tr = np.stack([VELO_TO_CAM] * S)
    tr[:, :, 3] = np.array([[0.05 * s, -0.08 + 0.01 * s, -0.27 - 0.02 * s] for s in range(S)])
    return tr


def _batch(rows, dev, fill=np.nan):
    lengths = [r.shape[0] for r in rows]
    out = np.full((len(rows), max(lengths), 4), fill, dtype=np.float32)
    for s, r in enumerate(rows):
        out[s, :r.shape[0]] = r
    return torch.from_numpy(out).to(dev), lengths


def _filter(rows, dataset, tr):
    if dataset == "kitti":
        return preprocess.transform_filter(rows, tr)
    return preprocess.kitti360_filter(rows, NEAR)


def _times_for(batch, lengths, dataset, tr, plant=True):
    """(S, R) fp64 times proportional to the row index, a different epoch per stream; with ``plant`` extreme and NaN times
    on the rows the filter drops and past each length: none of them may count."""
    S, R = batch.shape[:2]
    times = 1.6e9 + 10.0 * torch.arange(S, dtype=torch.float64)[:, None] + 0.1 * torch.arange(R, dtype=torch.float64)[None] / R
    times = times.to(batch.device)
    if plant:
        junk = torch.tensor([float("nan"), 1e300, -1e300, float("inf"), 0.0], dtype=torch.float64, device=batch.device)
        for s, n in enumerate(lengths):
            _, keep = _filter(batch[s, :n].contiguous(), dataset, None if tr is None else tr[s])
            drop = torch.cat([keep == 0, torch.ones(R - n, dtype=torch.bool, device=batch.device)])
            assert 0 < int((keep == 0).sum()) < n
            times[s, drop] = junk[torch.arange(int(drop.sum()), device=batch.device) % 5]
    return times


def _chain(batch, lengths, times, motion, dataset, tr, v, cap, width, npoints):
    """filter -> preprocess.deskew (the device op) -> [grid_sample] -> compact -> sampler -> gather, stream by stream.
    motion None: no de-skew step at all (the parent's chain)."""
    packed, counts, clouds = [], [], []
    for s, n in enumerate(lengths):
        xyz, keep = _filter(batch[s, :n].contiguous(), dataset, None if tr is None else tr[s])
        if motion is not None:
            xyz = preprocess.deskew(xyz, times[s, :n], motion[s], keep=keep)[0]
        if v is not None:
            keep = preprocess.grid_sample(xyz, v, keep=keep)[0][0]
        p, c = preprocess.compact(xyz[None], keep[None], width if v is not None else cap)
        idx = _ext.furthest_point_sampling(p, npoints)
        clouds.append(torch.gather(p, 1, idx.long().unsqueeze(-1).expand(-1, -1, 3)))
        packed.append(p)
        counts.append(c)
    return torch.cat(packed), torch.cat(counts), torch.cat(clouds)


def _small_rows():
    sw = _sweeps(12, 3, 46)                                                 # 64 beams x 46 azimuths: R <= 2944 rows
    return [sw[0], sw[1][:2000], sw[2][:1234]]


def _motion(names, dev):
    return torch.from_numpy(np.stack([model.IDENTITY if k == "identity" else model.MOTIONS[k] for k in names])).to(dev)


def _run(front, batch, lengths, times, motion):
    front.check_times(times, batch, "test")
    front.load(batch, lengths, front.check(batch, lengths, "test"), times)
    front.bufs["motion"].copy_(motion)
    return front.run()


@pytest.mark.parametrize("v", [None, 0.3], ids=["nogrid", "grid0.3"])
@pytest.mark.parametrize("dataset", ["kitti", "kitti360"])
def test_front_end_is_the_chain_of_ops(cuda, dataset, v):
    S, m, cap = 3, 256, 8192
    batch, lengths = _batch(_small_rows(), cuda)
    tr = _trs(S) if dataset == "kitti" else None
    times = _times_for(batch, lengths, dataset, tr)
    motion = _motion(["2deg", "w<0", "identity"], cuda)
    front = preprocess.SweepFrontEnd(S, m, dataset=dataset, capacity=cap, tr=tr, near_threshold=NEAR, voxel_size=v,
                                     deskew=True)
    want_p, want_c, want_clouds = _chain(batch, lengths, times, motion, dataset, tr, v, cap, cap, m)
    got = _run(front, batch, lengths, times, motion)
    assert torch.equal(front.bufs["packed"], want_p) and torch.equal(front.bufs["counts"], want_c)
    assert torch.equal(got, want_clouds)
    # the keep decision is the filter's, taken before the step: without a grid the counts are the parent's, and the
    # identity stream's rows are the parent's rows; the other streams' rows moved
    plain_p, plain_c, _ = _chain(batch, lengths, None, None, dataset, tr, v, cap, cap, m)
    if v is None:
        assert torch.equal(want_c, plain_c)
    assert torch.equal(want_p[2], plain_p[2]) and not torch.equal(want_p[0], plain_p[0]) and not torch.equal(want_p[1], plain_p[1])
    assert torch.isfinite(want_p).all()                                     # no planted time leaked into a coordinate
    # frames_to_clouds with the same arguments, frame by frame
    for s, n in enumerate(lengths):
        c, k = preprocess.frames_to_clouds(batch[s:s + 1, :n].contiguous(), m, dataset, tr=None if tr is None else tr[s],
                                           near_threshold=NEAR, cap=cap, voxel_size=v, times=times[s:s + 1, :n],
                                           motion=motion[s:s + 1])
        assert torch.equal(c, want_clouds[s:s + 1]) and int(k) == int(want_c[s])
    # a second, shorter set of sweeps with other motions through the same buffers, device lengths, fp32 times
    rows2 = [r[:r.shape[0] // 2] for r in _small_rows()][::-1]
    batch2, lengths2 = _batch(rows2, cuda)
    times2 = (_times_for(batch2, lengths2, dataset, tr, plant=False) - 1.6e9).float()
    motion2 = _motion(["identity", "90deg", "nq<1e-8"], cuda)
    want2 = _chain(batch2, lengths2, times2, motion2, dataset, tr, v, cap, cap, m)
    got2 = _run(front, batch2, torch.tensor(lengths2, dtype=torch.int32, device=cuda), times2, motion2)
    assert torch.equal(front.bufs["packed"], want2[0]) and torch.equal(front.bufs["counts"], want2[1])
    assert torch.equal(got2, want2[2])
    _lib.synchronize(cuda)


def test_front_end_on_a_sweep_wider_than_the_small_sampler(cuda):
    S, m, cap = 1, 256, 40000                                               # above 32768 rows: the cooperative, sorted sampler
    sweep = _sweeps(14, 2, 800)[0][:cap]
    assert sweep.shape[0] == cap
    batch, lengths = _batch([sweep], cuda)
    times = _times_for(batch, lengths, "kitti360", None)
    motion = _motion(["2deg"], cuda)
    front = preprocess.SweepFrontEnd(S, m, dataset="kitti360", capacity=cap, near_threshold=NEAR, deskew=True)
    want_p, want_c, want_clouds = _chain(batch, lengths, times, motion, "kitti360", None, None, cap, cap, m)
    got = _run(front, batch, lengths, times, motion)
    assert "order_ws" in front.bufs
    assert torch.equal(front.bufs["packed"], want_p) and torch.equal(front.bufs["counts"], want_c)
    assert torch.equal(got, want_clouds)
    _lib.synchronize(cuda)


@pytest.mark.parametrize("dataset", ["kitti", "kitti360"])
def test_with_deskew_off_the_clouds_are_the_parents(cuda, dataset):
    S, m = 3, 256
    batch, lengths = _batch(_small_rows(), cuda)
    tr = _trs(S) if dataset == "kitti" else None
    front = preprocess.SweepFrontEnd(S, m, dataset=dataset, capacity=4096, tr=tr, near_threshold=NEAR, deskew=False)
    front.load(batch, lengths, front.check(batch, lengths, "test"))
    got = front.run()
    assert "times" not in front.bufs and "motion" not in front.bufs
    for s, n in enumerate(lengths):
        c, k = preprocess.frames_to_clouds(batch[s:s + 1, :n].contiguous(), m, dataset, tr=None if tr is None else tr[s],
                                           near_threshold=NEAR, cap=4096)
        assert torch.equal(got[s:s + 1], c) and int(front.bufs["counts"][s]) == int(k)
    _lib.synchronize(cuda)


# ---- 3. streaming ------------------------------------------------------------------------------------------------------------

N, CAP, AZ = 1024, 8192, 78                                                  # 64 x 78 rays: at most 4992 rows per sweep


@functools.lru_cache(maxsize=None)
def _net(dev):
    net = PWCLONet(dict(num_input_channels=3, sequence_len=2, device=str(dev), scalar_last=False, log_mode="none"))
    params.fill_state_dict(net.state_dict())
    net = net.to(dev).eval()
    net.prepare_fused()
    return net


def _cm(clouds):
    return clouds.permute(0, 2, 1).contiguous()


def _ident(S, dev):
    return torch.from_numpy(np.stack([model.IDENTITY] * S)).to(dev)


def _stream_chain(batch, lengths, times, motion):
    return _chain(batch, lengths, times, motion, "kitti360", None, None, CAP, CAP, N)


@functools.lru_cache(maxsize=None)
def _lock_step(dev, graph):
    """Five sweeps on S = 2 streams through a de-skewing stream and, for the first two, a plain one.  Every check that
    needs the device state of the moment is made here; -> the poses, for the eager-against-replay comparison."""
    S, T = 2, 5
    seqs = [_sweeps(71 + s, T, AZ) for s in range(S)]
    net = _net(dev)
    fs = net._fused
    cfg = dict(dataset="kitti360", capacity=CAP, near_threshold=NEAR)
    raw = StreamingOdometry(net, streams=S, num_points=N, graph=graph, sweeps=dict(cfg, deskew=True))
    plain = StreamingOdometry(net, streams=S, num_points=N, graph=graph, sweeps=cfg)
    motion, prev, poses, moved = _ident(S, dev), None, [], []
    with torch.no_grad():
        for k in range(T):
            rows = [seqs[s][k][:seqs[s][k].shape[0] - 700 * ((k + s) % 3)] for s in range(S)]
            assert max(r.shape[0] for r in rows) <= 5000
            batch, lengths = _batch(rows, dev)
            times = _times_for(batch, lengths, "kitti360", None)
            want_p, want_c, clouds = _stream_chain(batch, lengths, times, motion)      # the previous call's level-1 rows
            plain_p, plain_c, plain_clouds = _stream_chain(batch, lengths, None, None)
            if k > 0:
                assert torch.equal(raw.motion(), motion), k
            got = raw.step_sweeps(batch, lengths if k % 2 else torch.tensor(lengths, dtype=torch.int32, device=dev),
                                  times=times)
            assert torch.equal(raw._front.bufs["packed"], want_p), k
            assert torch.equal(raw.survivor_counts(), want_c) and torch.equal(want_c, plain_c)   # the mask is the filter's
            if k < 2:                                                        # the identity: the deskew=False path, bit for bit
                ref = plain.step_sweeps(batch, lengths)
                assert torch.equal(raw._front.bufs["packed"], plain._front.bufs["packed"]) and torch.equal(clouds, plain_clouds)
                assert (got is None and ref is None) if k == 0 else torch.equal(got, ref)
            else:
                moved.append(not torch.equal(want_p, plain_p))
            if k > 0:
                assert torch.equal(got, fs(_cm(prev), _cm(clouds))), k
            motion = _ident(S, dev) if got is None else got[:, 0, :].clone()
            assert torch.equal(raw.motion(), motion), k
            poses.append(None if got is None else got.clone())
            prev = clouds
        assert all(moved) and len(moved) == 3                                # or the test proves nothing
        last = poses[-1][:, 0, :]
        assert float((last - _ident(S, dev)).abs().max()) > 1e-4             # the net's motion is no identity
        raw.reset()
        assert torch.equal(raw.motion(), _ident(S, dev))
        assert raw.step_sweeps(batch, lengths, times=times) is None          # the frame that primes replays the graph too
        assert torch.equal(raw.motion(), _ident(S, dev))
        assert torch.equal(raw._front.bufs["packed"], plain_p)               # de-skewed with the identity
    if graph:
        assert list(raw._graphs) == ["sweeps"] and raw.captures == 1
    _lib.synchronize(dev)
    return poses


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_lock_step_streams_use_the_previous_pose(cuda, graph):
    assert len(_lock_step(cuda, graph)) == 5


def test_lock_step_eager_equals_replay(cuda):
    a, b = _lock_step(cuda, True), _lock_step(cuda, False)
    assert a[0] is None and b[0] is None
    for x, y in zip(a[1:], b[1:]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_per_stream_motion_state_machine(cuda, graph):
    S = 3
    #            active     restart
    schedule = [((1, 1, 1), (0, 0, 0)),        # all prime: the identity
                ((1, 1, 1), (0, 0, 0)),        # first pairs, still the identity
                ((1, 0, 1), (0, 0, 0)),        # stream 1 idles: its motion is kept
                ((1, 1, 1), (0, 0, 1)),        # stream 1 comes back with the pre-idle pose; stream 2 restarts: the identity
                ((1, 1, 1), (0, 0, 0)),        # stream 2 after its prime: the identity again
                "reset 0",                     # reset(streams=[0])
                ((1, 1, 1), (0, 0, 0)),        # stream 0 primes: the identity
                ((1, 1, 1), (0, 0, 0))]        # and once more after the prime
    calls = [c for c in schedule if c != "reset 0"]
    seqs = [_sweeps(81 + s, len(calls), AZ) for s in range(S)]
    net = _net(cuda)
    fs = net._fused
    raw = StreamingOdometry(net, streams=S, num_points=N, graph=graph, per_stream=True,
                            sweeps=dict(dataset="kitti360", capacity=CAP, near_threshold=NEAR, deskew=True))
    ident = _ident(S, cuda)
    motion, have_prev, last = ident.clone(), [False] * S, [None] * S
    used_real, k = set(), 0
    with torch.no_grad():
        for item in schedule:
            if item == "reset 0":
                raw.reset(streams=[0])
                have_prev[0] = False
                motion[0] = ident[0]
                assert torch.equal(raw.motion(), motion)
                continue
            active, restart = item
            batch, lengths = _batch([seqs[s][k] for s in range(S)], cuda)
            times = _times_for(batch, lengths, "kitti360", None)
            primes = [bool(active[s]) and (bool(restart[s]) or not have_prev[s]) for s in range(S)]
            used = torch.stack([ident[s] if primes[s] else motion[s] for s in range(S)])
            want_p, _, clouds = _stream_chain(batch, lengths, times, used)
            got = raw.step_sweeps(batch, lengths, times=times, active=list(active), restart=list(restart)).clone()
            if all(last[s] is not None for s in range(S)):
                cur = torch.cat([clouds[s:s + 1] if active[s] else last[s] for s in range(S)])
                want = fs(_cm(torch.cat(last)), _cm(cur))
            for s in range(S):
                if not active[s]:
                    assert torch.equal(got[s, 0], ident[s])                  # idle: nothing moves, the motion included
                    continue
                assert torch.equal(raw._front.bufs["packed"][s], want_p[s]), (k, s)
                if primes[s]:
                    assert torch.equal(got[s, 0], ident[s])
                    motion[s] = ident[s]
                else:
                    assert torch.equal(got[s], want[s]), (k, s)
                    if not torch.equal(used[s], ident[s]):
                        used_real.add((k, s))
                    motion[s] = got[s, 0]
                have_prev[s] = True
                last[s] = clouds[s:s + 1]
            assert torch.equal(raw.motion(), motion), k
            k += 1
    # a real pose was used where the rule says so: stream 1 after its idle call (k = 3) among them
    assert (3, 1) in used_real and (2, 0) in used_real and (3, 2) not in used_real and (4, 2) not in used_real
    assert (5, 0) not in used_real and (6, 0) not in used_real and (6, 1) in used_real
    if graph:
        assert list(raw._graphs) == ["sweeps"] and raw.captures == 1
    _lib.synchronize(cuda)
