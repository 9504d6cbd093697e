"""Per-stream streaming odometry (``StreamingOdometry(per_stream=True)``): the two kernels alone
against the host model of tests/stream_mask_model.py, then the mode itself -- bit for bit the lock-step object when every
stream is active, and under dropouts and restarts bit for bit the pair forward on (each stream's last delivered frame,
its new frame), through one captured graph."""
import functools

import numpy as np
import pytest
import torch

import stream_mask_model as model
from oracle import params
from pwclonet_pylidarslam_amd import _lib, evaluation, fused, preprocess, synthetic
from pwclonet_pylidarslam_amd.odometry import StreamingOdometry
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet

pytestmark = pytest.mark.gpu

N = 1024
IDENT = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]           # [tx ty tz qw qx qy qz]


@functools.lru_cache(maxsize=None)
def _net_cached(dev, dtype):
    net = PWCLONet(dict(num_input_channels=3, sequence_len=2, device=str(dev), scalar_last=False, log_mode="none"))
    params.fill_state_dict(net.state_dict())
    net = net.to(dev).eval()
    net.prepare_fused(dtype=dtype)
    return net


def _net(dev, dtype=None):
    return _net_cached(dev, dtype)


@functools.lru_cache(maxsize=None)
def _host_streams(seed, n, t, s):
    return np.stack([synthetic.kitti_like_sequence(seed + i, n, t)[0] for i in range(s)], axis=1)


def _streams(seed, n, t, s, dev):
    """S independent sequences of T frames -> (T, S, n, 4): element k is the frame batch of call k."""
    return torch.from_numpy(_host_streams(seed, n, t, s)).to(dev)


def _cm(frames):
    return frames[:, :, :3].permute(0, 2, 1).contiguous()


def _i32(values, dev):
    return torch.tensor([int(v) for v in values], dtype=torch.int32, device=dev)


# ---- 1. the kernels alone ----------------------------------------------------------------------------------------------

def test_handover_kernel_moves_active_streams_only(cuda):
    S, guard = 5, 64
    active = _i32([1, 0, 1, 1, 0], cuda)
    # (bytes per stream, byte offset of both bases, extra destination stride).  16-byte path: 48 B, 40000 B (more than one
    # 16 KiB chunk, no multiple of it), 1 MiB + 16 KiB + 32 B (past the grid's 64 chunks: the loop takes a second round);
    # 4-byte path: 20004 B (size), 4096 B at a base 4 bytes off, 20 B; strided destination rows as the raw sweeps have.
    cases = [(48, 0, 0), (40000, 0, 0), (1024 * 1024 + 16384 + 32, 0, 0), (20004, 0, 0), (4096, 4, 0), (20, 0, 0),
             (4096, 0, 4096 + 32), (36, 0, 12)]
    g = torch.Generator(device="cpu").manual_seed(5)
    bufs, segs, dstr, sstr = [], [], [], []
    for nbytes, off, extra in cases:
        stride = nbytes + extra
        src = torch.randint(0, 256, (off + S * nbytes,), dtype=torch.uint8, generator=g).to(cuda)
        dst = torch.full((off + S * stride + guard,), 0xA5, dtype=torch.uint8, device=cuda)
        assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
        bufs.append((src, dst))
        segs.append((dst.data_ptr() + off, src.data_ptr() + off, nbytes))
        dstr.append(stride)
        sstr.append(nbytes)
    fused.masked_copy(segs, active, dst_strides=dstr, src_strides=sstr)
    _lib.synchronize(cuda)
    for (nbytes, off, extra), (src, dst) in zip(cases, bufs):
        stride = nbytes + extra
        want = torch.full_like(dst, 0xA5)
        for s in range(S):
            if int(active[s]):
                want[off + s * stride:off + s * stride + nbytes] = src[off + s * nbytes:off + (s + 1) * nbytes]
        assert torch.equal(dst, want), (nbytes, off, extra)        # active: the source's bytes; the rest and the guard: untouched
    # densely packed streams (no strides given), every stream idle, and a refused table
    src, dst = bufs[1][0], torch.zeros_like(bufs[1][0])
    fused.masked_copy([(dst.data_ptr(), src.data_ptr(), 40000)], active)
    fused.masked_copy([(dst.data_ptr(), src.data_ptr(), 40000)], _i32([0] * S, cuda))
    _lib.synchronize(cuda)
    for s in range(S):
        got = dst[s * 40000:(s + 1) * 40000]
        assert torch.equal(got, src[s * 40000:(s + 1) * 40000]) if int(active[s]) else not got.any()
    with pytest.raises(ValueError, match="segments"):
        fused.masked_copy([(dst.data_ptr(), src.data_ptr(), 16)] * 33, active)
    with pytest.raises(RuntimeError, match="4-byte"):
        fused.masked_copy([(dst.data_ptr(), src.data_ptr(), 18)], active)


def test_append_kernel_follows_the_model(cuda):
    S, cap = 4, 6
    m = model.StreamMaskModel(S, cap)
    z = lambda: torch.zeros((S,), dtype=torch.int32, device=cuda)
    have_prev, count, valid = z(), z(), z()
    overflow = torch.zeros((1,), dtype=torch.int32, device=cuda)
    rel = torch.full((cap, S, 4, 4), -7.0, dtype=torch.float64, device=cuda)
    abs_ = torch.full((cap, S, 4, 4), -7.0, dtype=torch.float64, device=cuda)
    want_rel, want_abs = rel.clone(), abs_.clone()
    eye = torch.eye(4, dtype=torch.float64, device=cuda)
    g = torch.Generator(device="cpu").manual_seed(9)
    for call, (active, restart) in enumerate(model.SCHEDULE):
        pose = torch.randn((S, 4, 7), generator=g).to(cuda)
        given = pose.clone()
        mats = evaluation.rows_to_transforms(given[:, 0, :])
        act, rst = _i32(active, cuda), _i32(restart, cuda)       # both alive until the launch: two different buffers
        _lib.call("stream_append_masked_kernel_wrapper", cuda, S, cap, act.data_ptr(), rst.data_ptr(), pose.data_ptr(),
                  rel.data_ptr(), abs_.data_ptr(), have_prev.data_ptr(), count.data_ptr(), valid.data_ptr(),
                  overflow.data_ptr())
        out = m.step(active, restart)
        _lib.synchronize(cuda)
        assert have_prev.tolist() == m.have_prev and count.tolist() == m.count and valid.tolist() == m.valid, call
        for s, (kind, row, _) in enumerate(out):
            if kind == model.PAIR:
                assert torch.equal(pose[s], given[s])                          # a real pair keeps its rows
                if row is not None:
                    want_rel[row, s] = mats[s]                                 # bitwise rows_to_transforms
                    prod = want_abs[row - 1, s] @ mats[s]
                    assert torch.allclose(abs_[row, s], prod, rtol=1e-12, atol=1e-12)
                    want_abs[row, s] = abs_[row, s]
            else:
                assert pose[s].tolist() == [IDENT] * 4, (call, s)
                if kind == model.PRIME:
                    want_rel[0, s] = eye
                    want_abs[0, s] = eye
        assert torch.equal(rel, want_rel) and torch.equal(abs_, want_abs), call     # every other row: untouched
        assert int(overflow.item()) == m.overflow
    assert m.count == [2, 5, 4, 3] and m.overflow == 0
    # a full trajectory: stream 1 (count 5 of 6) takes one more pair, then the next writes nothing and raises the flag
    for _ in range(2):
        pose = torch.randn((S, 4, 7), generator=g).to(cuda)
        before = (rel.clone(), abs_.clone())
        act, rst = _i32([0, 1, 0, 0], cuda), _i32([0] * S, cuda)
        _lib.call("stream_append_masked_kernel_wrapper", cuda, S, cap, act.data_ptr(), rst.data_ptr(), pose.data_ptr(),
                  rel.data_ptr(), abs_.data_ptr(), have_prev.data_ptr(), count.data_ptr(), valid.data_ptr(),
                  overflow.data_ptr())
        m.step([0, 1, 0, 0], [0] * S)
        _lib.synchronize(cuda)
        assert count.tolist() == m.count and valid.tolist() == m.valid and int(overflow.item()) == m.overflow
    assert m.overflow == 1 and m.count[1] == cap
    assert torch.equal(rel, before[0]) and torch.equal(abs_, before[1])


# ---- 2. every stream active: the lock-step object ------------------------------------------------------------------------

@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_all_active_is_bitwise_the_lock_step_stream(cuda, graph):
    S, T = 3, 5
    seq = _streams(3, N, T, S, cuda)
    net = _net(cuda)
    lock = StreamingOdometry(net, streams=S, graph=graph)
    per = StreamingOdometry(net, streams=S, graph=graph, per_stream=True)
    ident = torch.tensor(IDENT, device=cuda).expand(S, 4, 7)
    with torch.no_grad():
        for k in range(T):
            want = lock.step(seq[k])
            got = per.step(seq[k]) if k % 2 else per.step(seq[k], active=[1] * S, restart=torch.zeros(S, device=cuda).bool())
            if k == 0:
                assert want is None and torch.equal(got, ident) and per.valid().tolist() == [0] * S
            else:
                assert torch.equal(got, want), k
                assert per.valid().tolist() == [1] * S
    assert per.frame_counts().tolist() == [T] * S
    for i in range(S):
        assert torch.equal(per.relative_poses(stream=i), lock.relative_poses()[:, i])
        assert torch.equal(per.trajectory(stream=i), lock.trajectory()[:, i])
    assert per.captures == (1 if graph else 0) and not per.overflowed()


# ---- 3. ragged schedule ---------------------------------------------------------------------------------------------------

# stream 0 always active; stream 1 skips calls 2 and 3; stream 2 first appears at call 1 and restarts at call 5
RAGGED = [((1, 1, 0), (0, 0, 0)), ((1, 1, 1), (0, 0, 0)), ((1, 0, 1), (0, 0, 0)), ((1, 0, 1), (0, 0, 0)),
          ((1, 1, 1), (0, 0, 0)), ((1, 1, 1), (0, 0, 1)), ((1, 1, 1), (0, 0, 0))]


def _run_ragged(cuda, so, fs, seq, schedule, n, device_masks=False):
    """Run ``schedule`` on ``so`` and check every call against the model and the pair forward.  -> per stream the
    delivered call numbers of its current sequence, and the poses of its valid rows."""
    S = so.streams
    m = model.StreamMaskModel(S, so.max_frames)
    ident = torch.tensor(IDENT, device=cuda).expand(4, 7)
    last = [None] * S                                 # each stream's last delivered frame
    delivered = [[] for _ in range(S)]
    rows = [[] for _ in range(S)]
    graphs_after_first = None
    for k, (active, restart) in enumerate(schedule):
        frames = seq[k].clone()
        for s in range(S):
            if not active[s]:
                frames[s] = float("nan")              # an idle stream's row is never read
        if device_masks:
            pose = so.step(frames, active=_i32(active, cuda), restart=torch.tensor(restart, device=cuda).bool())
        else:
            pose = so.step(frames, active=list(active), restart=[bool(r) for r in restart])
        out = m.step(active, restart)
        assert pose.shape == (S, 4, 7) and torch.isfinite(pose).all()
        assert so.valid().tolist() == m.valid and so.frame_counts().tolist() == m.count, k
        # the pair forward at batch S on (last delivered frame, new frame); other rows: any finite pair
        f1 = torch.stack([last[s] if out[s][0] == model.PAIR else seq[k][s] for s in range(S)])
        f2 = torch.stack([seq[k][s] for s in range(S)])
        ref = fs(_cm(f1[:, :n]), _cm(f2[:, :n]))
        for s, (kind, row, prev) in enumerate(out):
            if kind == model.PAIR:
                assert prev == delivered[s][-1]
                assert torch.equal(pose[s], ref[s]), (k, s)
                rows[s].append(pose[s, 0].clone())
            else:
                assert torch.equal(pose[s], ident), (k, s)
            if kind == model.PRIME:
                delivered[s], rows[s] = [], []
            if active[s]:
                last[s] = seq[k][s]
                delivered[s].append(k)
        if k == 0:
            graphs_after_first = so.captures
    assert so.captures == graphs_after_first == (1 if so.graph else 0)      # one graph serves every call
    assert so.frame_counts().tolist() == [len(d) for d in delivered]
    return delivered, rows


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_ragged_schedule(cuda, graph):
    S, T = 3, len(RAGGED)
    seq = _streams(23, N, T, S, cuda)
    net = _net(cuda)
    fs = net._fused
    so = StreamingOdometry(net, streams=S, graph=graph, per_stream=True)
    lock = StreamingOdometry(net, streams=S, graph=graph)
    with torch.no_grad():
        delivered, rows = _run_ragged(cuda, so, fs, seq, RAGGED, N, device_masks=graph)
        assert delivered == [[0, 1, 2, 3, 4, 5, 6], [0, 1, 4, 5, 6], [5, 6]]
        eye = torch.eye(4, dtype=torch.float64, device=cuda)
        for i in range(S):
            rel, traj = so.relative_poses(stream=i), so.trajectory(stream=i)
            assert rel.shape == traj.shape == (len(delivered[i]), 4, 4)
            assert torch.equal(rel[0], eye) and torch.equal(traj[0], eye)
            assert torch.equal(rel[1:], evaluation.rows_to_transforms(torch.stack(rows[i])))
            want = [eye]
            for k in range(1, rel.shape[0]):
                want.append(want[-1] @ rel[k])
            assert torch.allclose(traj, torch.stack(want), rtol=1e-12, atol=1e-12)
            # the lock-step object fed stream i's delivered frames in all its rows
            lock.reset()
            for k in delivered[i]:
                lock.step(seq[k][i][None].expand(S, -1, -1).contiguous())
            assert torch.equal(traj, lock.trajectory()[:, i])
            assert torch.equal(rel, lock.relative_poses()[:, i])
        # reset(streams=[1]): stream 1 alone restarts on its next delivered frame, also after idling a call; until then
        # its counter and trajectory still show the old sequence
        so.reset(streams=[1])
        assert so.frame_counts().tolist() == [7, 5, 2]
        pose = so.step(seq[0], active=[1, 0, 1])
        assert so.valid().tolist() == [1, 0, 1] and so.frame_counts().tolist() == [8, 5, 3]
        assert so.trajectory(stream=1).shape == (5, 4, 4)
        pose = so.step(seq[1], active=[0, 1, 1])
        assert so.valid().tolist() == [0, 0, 1] and so.frame_counts().tolist() == [8, 1, 4]
        assert torch.equal(pose[1], torch.tensor(IDENT, device=cuda).expand(4, 7))
        so.reset(streams=torch.tensor([True, False, False], device=cuda))        # a device mask: bool
        pose = so.step(seq[2], active=[1, 1, 1])
        assert so.valid().tolist() == [0, 1, 1] and so.frame_counts().tolist() == [1, 2, 5]
        with pytest.raises(ValueError, match="bool"):
            so.reset(streams=torch.tensor([1, 0, 0], device=cuda))
        so.reset()
        assert so.frames_seen == 0 and so.frame_counts().tolist() == [0, 0, 0]
        pose = so.step(seq[2], active=[0, 1, 0])
        assert so.valid().tolist() == [0, 0, 0] and so.frame_counts().tolist() == [0, 1, 0]
    assert so.captures == (1 if graph else 0) and not so.overflowed()
    _lib.synchronize(cuda)


# ---- 4. a state with kept search structures, fp32 and bf16 ------------------------------------------------------------------

def _kept_levels(fs, frames, n):
    state = fs.stream_prime(frames, n)
    return [lvl for lvl in fused.FrameState.FRAME1_BUILT if lvl in state.built], state


@pytest.mark.parametrize("dtype", [None, "bf16"], ids=["fp32", "bf16"])
def test_gap_with_kept_structures(cuda, dtype):
    """The handover of a state that holds kept search structures (both workspace sections) and, with bf16 packing, bf16
    cost-volume products.  Which pyramid clouds keep a structure follows the network's fixed sample counts, not
    ``num_points``: the test asserts that its size keeps exactly the levels the flagship size (8192 points) keeps."""
    S, n = 2, N
    schedule = [((1, 1), (0, 0)), ((1, 0), (0, 0)), ((1, 1), (0, 0)), ((1, 1), (0, 0))]
    seq = _streams(43, n, len(schedule), S, cuda)
    net = _net(cuda, dtype)
    fs = net._fused
    with torch.no_grad():
        kept, state = _kept_levels(fs, seq[0], n)
        big = torch.from_numpy(synthetic.kitti_like_sequence(7, 8192, 2)[0][:1]).to(cuda)
        assert kept and kept == _kept_levels(fs, big, 8192)[0]
        segs = state.frame1_segments(state.frame1_buffers())
        assert len(segs) == len(state.frame1_tensors()) + len(kept)            # every kept workspace: two segments
        assert sum(b for _, _, b in segs) * S == state.frame1_bytes()
        if dtype == "bf16":
            assert any(u.dtype == torch.bfloat16 for u, _, _ in state.cv.values())
        so = StreamingOdometry(net, streams=S, graph=True, per_stream=True)
        delivered, _ = _run_ragged(cuda, so, fs, seq, schedule, n)
    assert delivered == [[0, 1, 2, 3], [0, 2, 3]]
    _lib.synchronize(cuda)


# ---- 5. raw mode ----------------------------------------------------------------------------------------------------------

def test_raw_mode_idle_stream_keeps_its_sweep(cuda):
    # the front end accepts any capacity >= the rows of a sweep; the smallest sweeps the generator makes that still keep
    # n = 1024 survivors are 64 beams x 256 azimuths = 16384 rays, so that is the capacity (asserted below)
    S, T, cap, n = 2, 4, 64 * 256, N
    sweeps = [synthetic.raw_sweep_sequence(61 + s, T, n_azimuth=256)[0] for s in range(S)]
    assert cap // 2 < max(sw.shape[0] for seq_ in sweeps for sw in seq_) <= cap
    net = _net(cuda)
    raw = StreamingOdometry(net, streams=S, num_points=n, graph=True, per_stream=True,
                            sweeps=dict(dataset="kitti360", capacity=cap))
    ref = StreamingOdometry(net, streams=S, num_points=n, graph=True, per_stream=True)
    schedule = [(1, 1), (1, 0), (1, 1), (1, 1)]                 # stream 1 idles at call 1, then delivers a shorter sweep
    with torch.no_grad():
        for k, active in enumerate(schedule):
            rows = [sweeps[s][k] for s in range(S)]
            if k == 2:
                rows[1] = rows[1][:rows[1].shape[0] - 1500]
            lengths = [r.shape[0] for r in rows]
            assert max(lengths) <= cap
            batch = np.full((S, max(lengths), 4), np.nan, dtype=np.float32)
            for s, r in enumerate(rows):
                batch[s, :r.shape[0]] = r
            batch = torch.from_numpy(batch).to(cuda)
            clouds, counts = zip(*[preprocess.frames_to_clouds(batch[s:s + 1, :lengths[s]].contiguous(), n, "kitti360",
                                                               cap=cap) for s in range(S)])
            clouds, counts = torch.cat(clouds), torch.cat(counts)
            before = None if k == 0 else raw.survivor_counts().clone()
            lens = torch.tensor(lengths, dtype=torch.int32, device=cuda) if k % 2 else lengths
            got = raw.step_sweeps(batch, lens, active=list(active))
            want = ref.step(clouds, active=list(active))
            assert torch.equal(got, want), k
            assert raw.valid().tolist() == ref.valid().tolist() == ([0, 0] if k == 0 else list(active))
            for s in range(S):
                if active[s]:
                    assert int(raw.survivor_counts()[s]) == int(counts[s])
                else:
                    assert int(raw.survivor_counts()[s]) == int(before[s])     # the sweep it delivered last
    assert raw.frame_counts().tolist() == ref.frame_counts().tolist() == [4, 3]
    assert list(raw._graphs) == ["sweeps"] and raw.captures == 1
    _lib.synchronize(cuda)


# ---- 6. refusals before any launch ------------------------------------------------------------------------------------------

def test_refused_inputs_raise_before_any_launch(cuda):
    S = 3
    seq = _streams(3, N, 2, S, cuda)
    so = StreamingOdometry(_net(cuda), streams=S, graph=True, per_stream=True)
    with torch.no_grad():
        with pytest.raises(ValueError, match="active"):
            so.step(seq[0], active=[1, 0])
        with pytest.raises(ValueError, match="restart"):
            so.step(seq[0], restart=torch.zeros(S + 1, dtype=torch.int32, device=cuda))
        with pytest.raises(ValueError, match="at least one active"):
            so.step(seq[0], active=[0, 0, 0])
        assert so.frames_seen == 0 and so._slot is None and so.captures == 0 and not so._graphs     # nothing ran
        with pytest.raises(ValueError, match="stream=i"):
            so.relative_poses()
        so.step(seq[0], active=[0, 1, 0])
        with pytest.raises(ValueError, match="active"):
            so.step(seq[1], active=[1, 0, 1, 1])
        with pytest.raises(ValueError, match="stream=i"):
            so.trajectory()
        pose = so.step(seq[1], active=[0, 0, 0])               # later calls may idle every stream
        assert so.valid().tolist() == [0, 0, 0] and so.frame_counts().tolist() == [0, 1, 0]
        assert torch.equal(pose, torch.tensor(IDENT, device=cuda).expand(S, 4, 7))
    assert so.frames_seen == 2 and so.captures == 1
