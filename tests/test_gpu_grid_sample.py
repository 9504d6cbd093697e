"""Voxel grid sampling on the device, everything compared exactly: the stand-alone op against the
NumPy model of tests/grid_sample_model.py, a persistent workspace, the raw front end with a grid against filter -> model ->
compaction -> sampler, streaming odometry on grid-sampled sweeps against the pair forward, and the unchanged default."""
import functools

import numpy as np
import pytest
import torch

import grid_sample_model as model
from oracle import params
from pwclonet_pylidarslam_amd import _lib, preprocess, synthetic
from pwclonet_pylidarslam_amd.odometry import StreamingOdometry
from pwclonet_pylidarslam_amd.pointnet2_ops import _ext
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet

pytestmark = pytest.mark.gpu

NEAR = 30.0
VELO_TO_CAM = np.array([[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0], [1.0, 0.0, 0.0, 0.0]])


# ---- 1. the stand-alone op against the model -------------------------------------------------------------------------------

def _inputs(n, v, seed):
    """name -> (n, 3) float32 cloud; every kind the op must get right at this n and voxel size."""
    r = np.random.default_rng([seed, n])
    slab = r.random((n, 3)) * [160.0, 160.0, 4.0] - [80.0, 80.0, 2.0]
    cells = r.integers(-40, 40, (max(1, n // 8), 3))
    lattice = (cells[r.integers(0, cells.shape[0], n)] + r.uniform(-0.4, 0.4, (n, 3))) * v        # ~8 rows per voxel
    one = (np.array([7.0, -3.0, 1.0]) + r.uniform(-0.4, 0.4, (n, 3))) * v
    i = np.arange(n)
    distinct = np.stack([i - n // 2, i % 7, -(i % 3)], axis=1) * v
    origin = slab.copy()
    origin[::3] = r.uniform(-0.4, 0.4, (len(origin[::3]), 3)) * v                                 # h = 0, many times
    origin[n // 2] = [-0.0, 0.0, -0.0]
    bad = slab.astype(np.float32)
    bad[n // 2, 0] = np.nan
    bad[n // 3, 2] = np.inf
    bad[(2 * n) // 3, 1] = -np.inf
    bad[n - 1] = [3.0e9 * v, 0.0, 0.0]                                                            # |p / v| >= 2^31
    return {"slab": slab.astype(np.float32), "lattice": lattice.astype(np.float32), "one": one.astype(np.float32),
            "distinct": distinct.astype(np.float32), "origin": origin.astype(np.float32), "bad": bad}


def _op(points, v, lengths=None, keep=None, dev=None, **kw):
    """numpy in, numpy out through preprocess.grid_sample."""
    pts = torch.from_numpy(points).to(dev)
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=dev)
    kp = None if keep is None else torch.from_numpy(keep).to(dev)
    got_keep, got_counts = preprocess.grid_sample(pts, v, lengths=ln, keep=kp, **kw)
    return got_keep.cpu().numpy(), got_counts.cpu().numpy()


def _with_stride(clouds, stride, seed):
    """(b, n, 3) -> (b, n, stride): a fourth column of noise that must not matter."""
    if stride == 3:
        return clouds
    extra = np.random.default_rng(seed).random(clouds.shape[:2] + (1,)).astype(np.float32)
    return np.concatenate([clouds, extra], axis=2)


@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("v", [0.2, 0.3, 0.5])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1024, 1025, 5000])
def test_op_equals_the_model(cuda, n, v, stride):
    kinds = _inputs(n, v, 7)
    clouds = _with_stride(np.stack(list(kinds.values())), stride, n)        # one launch: a cloud per kind
    want_keep, want_counts = model.grid_keep_batch(clouds, v)
    got_keep, got_counts = _op(clouds, v, dev=cuda)
    for c, name in enumerate(kinds):
        assert np.array_equal(got_keep[c], want_keep[c]), (name, np.flatnonzero(got_keep[c] != want_keep[c])[:8])
    assert np.array_equal(got_counts, want_counts)
    by = dict(zip(kinds, want_counts))
    assert by["one"] == 1 and by["distinct"] == n                           # the inputs are what their names say
    if n >= 1024:
        assert n // 16 < by["lattice"] <= n // 8 and by["slab"] > n // 2
        assert by["bad"] <= n - 4
    _lib.synchronize(cuda)


@pytest.mark.parametrize("v", [0.5, 0.25])
def test_rows_on_half_voxel_boundaries_go_to_the_even_voxel(cuda, v):
    k = np.arange(-6, 6)
    half = (k + 0.5) * v                                                    # exact in fp32 and fp64: every quotient is k + 0.5
    x, y, z = np.meshgrid(half, half, half, indexing="ij")
    pts = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.float32)
    assert np.array_equal(pts.astype(np.float64) / v, np.floor(pts.astype(np.float64) / v) + 0.5)
    got_keep, got_counts = _op(pts[None], v, dev=cuda)
    want = model.grid_keep(pts, v)
    assert np.array_equal(got_keep[0], want)
    # per axis the 12 half-way values fall on the 7 even integers -6 .. 6, so 7^3 voxels hold the 12^3 rows
    assert int(got_counts[0]) == want.sum() == 7 ** 3
    # four rows by hand, scaled to this voxel: quotients 0.5, 1.5, -0.5, 2.5 -> 0, 2, -0, 2
    four = np.zeros((4, 3), dtype=np.float32)
    four[:, 0] = np.array([0.5, 1.5, -0.5, 2.5]) * v
    assert _op(four[None], v, dev=cuda)[0][0].tolist() == [1, 1, 0, 0]
    _lib.synchronize(cuda)


@pytest.mark.parametrize("stride", [3, 4])
def test_three_clouds_of_different_lengths(cuda, stride):
    n, v, lengths = 3000, 0.3, [3000, 1, 1777]
    kinds = _inputs(n, v, 21)
    clouds = np.stack([kinds["lattice"], kinds["slab"], kinds["origin"]])
    for c, ln in enumerate(lengths):
        clouds[c, ln:] = np.nan if c else 0.0                               # rows past a length are never read as candidates
    clouds[2, 1777:] = clouds[2, :n - 1777]                                 # ... even when they repeat rows before it
    clouds = _with_stride(clouds, stride, 3)
    want_keep, want_counts = model.grid_keep_batch(clouds, v, lengths=lengths)
    got_keep, got_counts = _op(clouds, v, lengths=lengths, dev=cuda)
    assert np.array_equal(got_keep, want_keep) and np.array_equal(got_counts, want_counts)
    assert want_counts[1] == 1 and not got_keep[1, 1:].any() and not got_keep[2, 1777:].any()
    _lib.synchronize(cuda)


def test_keep_in_mask_decides_the_candidates(cuda):
    n, v = 5000, 0.3
    r = np.random.default_rng(5)
    clouds = np.stack([_inputs(n, v, 31)["lattice"], _inputs(n, v, 32)["lattice"]])
    keep = (r.random((2, n)) < 0.6).astype(np.int32)
    keep[1, :2500] = 0                                                      # every voxel's first rows masked out
    want_keep, want_counts = model.grid_keep_batch(clouds, v, keep=keep)
    got_keep, got_counts = _op(clouds, v, keep=keep, dev=cuda)
    assert np.array_equal(got_keep, want_keep) and np.array_equal(got_counts, want_counts)
    assert not (got_keep & (1 - keep)).any()
    free = model.grid_keep_batch(clouds, v)[0]
    assert (free != want_keep).any()                                        # the mask changed who wins
    # it composes with compact: the winners' rows, in row order
    packed, counts = preprocess.compact(torch.from_numpy(clouds).to(cuda), torch.from_numpy(got_keep).to(cuda), 1024)
    for c in range(2):
        rows = clouds[c][want_keep[c] != 0][:1024]
        assert int(counts[c]) == rows.shape[0] == min(1024, want_counts[c])
        assert np.array_equal(packed[c, :rows.shape[0]].cpu().numpy(), rows)
    _lib.synchronize(cuda)


def test_a_row_whose_hash_is_the_empty_slot_marker(cuda):
    q = model.solve_hash(model.EMPTY_KEY)
    assert q is not None, "no voxel within +-2^24 hashes to the marker"
    v = 1.0                                                                 # the coordinates are the voxel indices
    rest = _inputs(500, v, 41)["slab"]
    pts = np.concatenate([rest[:100], np.float32([q]), rest[100:], np.float32([q, q, [0, 0, 0]])]).astype(np.float32)
    h, ok = model.voxel_hash(pts, v)
    assert ok.all() and (h == model.EMPTY_KEY).sum() == 3 and h[100] == model.EMPTY_KEY
    got_keep, got_counts = _op(pts[None], v, dev=cuda)
    want = model.grid_keep(pts, v)
    assert np.array_equal(got_keep[0], want) and int(got_counts[0]) == want.sum()
    assert got_keep[0, 100] == 1 and not got_keep[0, -3:-1].any()
    _lib.synchronize(cuda)


# ---- 2. a persistent workspace -----------------------------------------------------------------------------------------------

def test_persistent_workspace_keeps_nothing_between_calls(cuda):
    v = 0.3
    big = np.stack([_inputs(5000, v, 51)["lattice"], _inputs(5000, v, 52)["origin"]])
    small = np.stack([_inputs(1300, v, 53)["lattice"], _inputs(1300, v, 54)["slab"]])
    ws = preprocess.grid_sample_workspace(2, 5000, cuda)
    ws.random_()                                                            # whatever the buffer held before
    first = _op(big, v, dev=cuda, workspace=ws)
    again = _op(big, v, dev=cuda, workspace=ws)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    assert np.array_equal(first[0], model.grid_keep_batch(big, v)[0])
    fresh = _op(small, v, lengths=[1300, 700], dev=cuda)
    reused = _op(small, v, lengths=[1300, 700], dev=cuda, workspace=ws)      # fewer rows, other data, the same buffer
    assert np.array_equal(reused[0], fresh[0]) and np.array_equal(reused[1], fresh[1])
    assert np.array_equal(reused[0], model.grid_keep_batch(small, v, lengths=[1300, 700])[0])
    _lib.synchronize(cuda)


# ---- 3. the raw front end ------------------------------------------------------------------------------------------------------

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


def _small_rows():
    sw = _sweeps(12, 3, 46)                                                 # 64 beams x 46 azimuths: R <= 2944 rows
    rows = [sw[0], sw[1][:2000], sw[2][:1234]]
    assert max(r.shape[0] for r in rows) <= 3000
    return rows


def _filter(rows, dataset, tr):
    if dataset == "kitti":
        return preprocess.transform_filter(rows, tr)
    return preprocess.kitti360_filter(rows, NEAR)


def _reference(batch, lengths, dataset, tr, v, width, npoints):
    """filter -> model grid on the kept rows -> compact -> sampler -> gather, stream by stream."""
    packed, counts, winners, clouds = [], [], [], []
    for s, n in enumerate(lengths):
        xyz, keep = _filter(batch[s, :n].contiguous(), dataset, None if tr is None else tr[s])
        if v is not None:
            won = model.grid_keep(xyz.cpu().numpy(), v, keep=keep.cpu().numpy())
            winners.append(int(won.sum()))
            keep = torch.from_numpy(won).to(batch.device)
        p, c = preprocess.compact(xyz[None], keep[None], width)
        idx = _ext.furthest_point_sampling(p, npoints)
        clouds.append(torch.gather(p, 1, idx.long().unsqueeze(-1).expand(-1, -1, 3)))
        packed.append(p)
        counts.append(c)
    return torch.cat(packed), torch.cat(counts), winners, torch.cat(clouds)


def _run(front, batch, lengths):
    front.load(batch, lengths, front.check(batch, lengths, "test"))
    return front.run()


@pytest.mark.parametrize("capacity, width", [(4096, None), (40000, 4096)], ids=["cap4096", "cap40000_width4096"])
@pytest.mark.parametrize("dataset", ["kitti", "kitti360"])
def test_front_end_with_a_grid(cuda, dataset, capacity, width):
    S, m, v = 3, 256, 0.3
    batch, lengths = _batch(_small_rows(), cuda)
    tr = _trs(S) if dataset == "kitti" else None
    front = preprocess.SweepFrontEnd(S, m, dataset=dataset, capacity=capacity, tr=tr, near_threshold=NEAR, voxel_size=v,
                                     voxel_capacity=width)
    wide = capacity if width is None else width
    want_p, want_c, want_w, want_clouds = _reference(batch, lengths, dataset, tr, v, wide, m)
    assert min(want_w) > 0
    got = _run(front, batch, lengths)
    assert front.bufs["packed"].shape == (S, wide, 3)
    assert torch.equal(front.bufs["packed"], want_p)
    assert torch.equal(front.bufs["counts"], want_c) and front.voxel_counts().tolist() == want_w == want_c.tolist()
    assert torch.equal(got, want_clouds)
    assert "tmp" not in front.bufs and "order_ws" not in front.bufs         # the small width chose the sampler
    # a second, shorter set of sweeps through the same buffers (table, packed rows): nothing of the first survives
    rows2 = [r[:r.shape[0] // 2] for r in _small_rows()][::-1]
    batch2, lengths2 = _batch(rows2, cuda)
    tr2 = None if tr is None else tr
    want2 = _reference(batch2, lengths2, dataset, tr2, v, wide, m)
    got2 = _run(front, batch2, torch.tensor(lengths2, dtype=torch.int32, device=cuda))      # device lengths
    assert torch.equal(front.bufs["packed"], want2[0]) and front.voxel_counts().tolist() == want2[2]
    assert torch.equal(got2, want2[3])
    # frames_to_clouds with the same arguments, frame by frame
    for s, n in enumerate(lengths):
        c, k = preprocess.frames_to_clouds(batch[s:s + 1, :n].contiguous(), m, dataset, tr=None if tr is None else tr[s],
                                           near_threshold=NEAR, cap=capacity, voxel_size=v, voxel_capacity=width)
        assert torch.equal(c, want_clouds[s:s + 1]) and int(k) == want_w[s]
    _lib.synchronize(cuda)


@pytest.mark.parametrize("dataset", ["kitti", "kitti360"])
def test_winners_beyond_voxel_capacity_are_dropped_in_row_order(cuda, dataset):
    S, m, v, width = 3, 64, 0.3, 64
    batch, lengths = _batch(_small_rows(), cuda)
    tr = _trs(S) if dataset == "kitti" else None
    front = preprocess.SweepFrontEnd(S, m, dataset=dataset, capacity=4096, tr=tr, near_threshold=NEAR, voxel_size=v,
                                     voxel_capacity=width)
    full_p, _, want_w, _ = _reference(batch, lengths, dataset, tr, v, 4096, m)
    want_p, want_c, _, want_clouds = _reference(batch, lengths, dataset, tr, v, width, m)
    assert min(want_w) > width                                              # every stream overflows
    got = _run(front, batch, lengths)
    assert torch.equal(front.bufs["packed"], full_p[:, :width]) and torch.equal(front.bufs["packed"], want_p)
    assert front.voxel_counts().tolist() == want_w                          # the true number
    assert front.bufs["counts"].tolist() == want_c.tolist() == [width] * S  # the clamped one
    assert torch.equal(got, want_clouds)
    _lib.synchronize(cuda)


@pytest.mark.parametrize("dataset", ["kitti", "kitti360"])
def test_without_a_grid_the_clouds_are_the_parents(cuda, dataset):
    S, m = 3, 256
    batch, lengths = _batch(_small_rows(), cuda)
    tr = _trs(S) if dataset == "kitti" else None
    front = preprocess.SweepFrontEnd(S, m, dataset=dataset, capacity=4096, tr=tr, near_threshold=NEAR, voxel_size=None,
                                     voxel_capacity=None)
    got = _run(front, batch, lengths)
    assert front.voxel_counts() is None and "grid_ws" not in front.bufs
    for s, n in enumerate(lengths):
        c, k = preprocess.frames_to_clouds(batch[s:s + 1, :n].contiguous(), m, dataset, tr=None if tr is None else tr[s],
                                           near_threshold=NEAR, cap=4096)
        assert torch.equal(got[s:s + 1], c) and int(front.bufs["counts"][s]) == int(k)
    _lib.synchronize(cuda)


# ---- 4. streaming ------------------------------------------------------------------------------------------------------------

N, CAP, V = 1024, 64 * 256, 0.2        # tests/test_gpu_stream_mask.py's raw set-up; 0.2 m keeps more than N winners per sweep


@functools.lru_cache(maxsize=None)
def _net(dev):
    net = PWCLONet(dict(num_input_channels=3, sequence_len=2, device=str(dev), scalar_last=False, log_mode="none"))
    params.fill_state_dict(net.state_dict())
    net = net.to(dev).eval()
    net.prepare_fused()
    return net


def _cm(clouds):
    return clouds.permute(0, 2, 1).contiguous()


def _eager_clouds(batch, lengths, width):
    out = [preprocess.frames_to_clouds(batch[s:s + 1, :n].contiguous(), N, "kitti360", near_threshold=NEAR, cap=CAP,
                                       voxel_size=V, voxel_capacity=width) for s, n in enumerate(lengths)]
    return torch.cat([c for c, _ in out]), torch.cat([k for _, k in out])


def test_streaming_on_grid_sampled_sweeps_is_the_pair_forward(cuda):
    S, T, width = 2, 3, 4096
    seqs = [_sweeps(61 + s, T, 256) for s in range(S)]
    net = _net(cuda)
    fs = net._fused
    raw = StreamingOdometry(net, streams=S, num_points=N, graph=True,
                            sweeps=dict(dataset="kitti360", capacity=CAP, near_threshold=NEAR, voxel_size=V,
                                        voxel_capacity=width))
    prev = None
    with torch.no_grad():
        for k in range(T):                                                   # three sweeps, every length different
            rows = [seqs[s][k][:seqs[s][k].shape[0] - 1000 * ((k + s) % 3)] for s in range(S)]
            batch, lengths = _batch(rows, cuda)
            clouds, counts = _eager_clouds(batch, lengths, width)
            assert N < int(counts.min()) and int(counts.max()) < width
            lens = torch.tensor(lengths, dtype=torch.int32, device=cuda) if k % 2 else lengths
            got = raw.step_sweeps(batch, lens)
            assert torch.equal(raw.survivor_counts(), counts) and torch.equal(raw.voxel_counts(), counts)
            if k == 0:
                assert got is None
            else:
                assert torch.equal(got, fs(_cm(prev), _cm(clouds))), k
            prev = clouds
        raw.reset()
        assert raw.step_sweeps(batch, lens) is None                          # the frame that primes replays it too
    assert list(raw._graphs) == ["sweeps"] and raw.captures == 1
    _lib.synchronize(cuda)


def test_per_stream_streaming_with_an_idle_stream(cuda):
    S, T, width = 2, 4, 4096
    seqs = [_sweeps(61 + s, T, 256) for s in range(S)]
    net = _net(cuda)
    fs = net._fused
    raw = StreamingOdometry(net, streams=S, num_points=N, graph=True, per_stream=True,
                            sweeps=dict(dataset="kitti360", capacity=CAP, near_threshold=NEAR, voxel_size=V,
                                        voxel_capacity=width))
    schedule = [(1, 1), (1, 0), (1, 1), (1, 1)]                             # stream 1 idles at call 1, then comes back shorter
    last = [None] * S                                                       # each stream's last delivered cloud
    ident = torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], device=cuda).expand(4, 7)
    with torch.no_grad():
        for k, active in enumerate(schedule):
            rows = [seqs[s][k] for s in range(S)]
            if k == 2:
                rows[1] = rows[1][:rows[1].shape[0] - 1500]
            batch, lengths = _batch(rows, cuda)
            clouds, counts = _eager_clouds(batch, lengths, width)
            before = None if k == 0 else raw.voxel_counts().clone()
            got = raw.step_sweeps(batch, lengths, active=list(active))
            # the pair forward at the stream's batch size on (each stream's last delivered cloud, its new cloud); an idle
            # stream's row of it is not looked at
            if k > 0:
                cur = torch.cat([clouds[s:s + 1] if active[s] else last[s] for s in range(S)])
                want = fs(_cm(torch.cat(last)), _cm(cur))
            for s in range(S):
                if not active[s]:
                    assert torch.equal(got[s], ident) and int(raw.voxel_counts()[s]) == int(before[s])
                    continue
                assert int(raw.voxel_counts()[s]) == int(raw.survivor_counts()[s]) == int(counts[s])
                if last[s] is None:
                    assert torch.equal(got[s], ident)                        # primed
                else:
                    assert torch.equal(got[s], want[s]), (k, s)
                last[s] = clouds[s:s + 1]
            assert raw.valid().tolist() == ([0, 0] if k == 0 else list(active))
    assert raw.frame_counts().tolist() == [4, 3]
    assert list(raw._graphs) == ["sweeps"] and raw.captures == 1
    _lib.synchronize(cuda)
