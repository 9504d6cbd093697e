"""Streaming odometry (``FusedPWCLONet.stream_step``, ``odometry.StreamingOdometry``): one frame per call, the previous
frame's pyramid kept.  The bar is the fused pair forward at batch S on the same pairs: rows, every neighbour list and
the pair-stage intermediates bit-identical (any env switch, fp32 and bf16 packing), through graph replay too; the
device trajectories agree with the evaluation kernels."""
import functools

import numpy as np
import pytest
import torch

from oracle import params
from pwclonet_pylidarslam_amd import evaluation, synthetic
from pwclonet_pylidarslam_amd.odometry import PWCLONetOdometry, StreamingOdometry
from pwclonet_pylidarslam_amd.prediction import PWCLONetPredictionModule
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet

pytestmark = pytest.mark.gpu

# the env switches and bf16 packing of tests/test_gpu_sequence.py
SWITCHES = [("default", {}, None), ("hoist0", {"PWCLO_HOIST": "0"}, None), ("knn_reuse0", {"PWCLO_KNN_REUSE": "0"}, None),
            ("early_cv0", {"PWCLO_EARLY_CV": "0"}, None), ("pw_tail0", {"PWCLO_PW_TAIL": "0"}, None),
            ("head_warp0", {"PWCLO_HEAD_WARP": "0"}, None), ("bf16", {}, "bf16")]


def _net(dev, dtype=None, fused="auto"):
    net = PWCLONet(dict(num_input_channels=3, sequence_len=2, device=str(dev), scalar_last=False, log_mode="none",
                        fused=fused))
    params.fill_state_dict(net.state_dict())
    net = net.to(dev).eval()
    if fused != "off":
        net.prepare_fused(dtype=dtype)
    return net


@functools.lru_cache(maxsize=None)
def _host_streams(seed, n, t, s):
    return np.stack([synthetic.kitti_like_sequence(seed + i, n, t)[0] for i in range(s)], axis=1)


def _streams(seed, n, t, s, dev):
    """S independent sequences of T frames -> (T, S, n, 4): element k is the frame batch of step k."""
    return torch.from_numpy(_host_streams(seed, n, t, s)).to(dev)


def _cm(frames):
    """(B, N, c) point-major frames -> the pair forward's (B, 3, N) input."""
    return frames[:, :, :3].permute(0, 2, 1).contiguous()


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("name,env,dtype", SWITCHES, ids=[s[0] for s in SWITCHES])
def test_stream_is_bitwise_the_pair_forward(cuda, monkeypatch, name, env, dtype, S):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    seq = _streams(3, 4096, 9, S, cuda)                          # c = 4: every frame goes through the ingest kernel
    net = _net(cuda, dtype)
    fs = net._fused
    assert fs.hoist == (env.get("PWCLO_HOIST", "1") == "1")
    so = StreamingOdometry(net, streams=S, graph=False)
    with torch.no_grad():
        state = fs.stream_prime(seq[0], 4096)
        assert so.step(seq[0]) is None
        for k in range(1, seq.shape[0]):
            pose, inter, state = fs.stream_step(state, seq[k], 4096, return_intermediates=True)
            ref, inter_ref = fs(_cm(seq[k - 1]), _cm(seq[k]), return_intermediates=True)
            api = so.step(seq[k])
            assert pose.shape == (S, 4, 7)
            assert torch.equal(pose, ref), (name, S, k)
            assert torch.equal(api, ref), (name, S, k)
            assert sorted(inter["lists"]) == sorted(inter_ref["lists"])
            for key, idx in inter_ref["lists"].items():
                got = inter["lists"][key]
                if key.startswith("psa_"):      # pyramid lists: the pair forward holds both frames, the step the new one
                    assert torch.equal(got, idx[S:]), (key, k)
                else:
                    assert torch.equal(got, idx), (key, k)
            for key in ("x11", "f13", "flow", "emb1", "mask1"):
                assert torch.equal(inter[key], inter_ref[key]), (key, k)
    assert so.frames_seen == seq.shape[0]


def test_graph_replay_and_reset(cuda):
    """The captured graph gives the eager rows over 13 steps, then again on a second sequence after reset()."""
    net = _net(cuda)
    S = 2
    a = _streams(21, 4096, 13, S, cuda)
    b = _streams(41, 4096, 13, S, cuda)
    eager = StreamingOdometry(net, streams=S, graph=False)
    graphed = StreamingOdometry(net, streams=S, graph=True)
    with torch.no_grad():
        for seq in (a, b):
            eager.reset()
            graphed.reset()
            assert eager.step(seq[0]) is None and graphed.step(seq[0]) is None
            for k in range(1, seq.shape[0]):
                want = eager.step(seq[k]).clone()
                got = graphed.step(seq[k]).clone()
                assert torch.equal(got, want), k
            assert torch.equal(graphed.relative_poses(), eager.relative_poses())
            assert torch.equal(graphed.trajectory(), eager.trajectory())
    assert graphed.handover_bytes > 0 and len(graphed._graphs) == 1 and graphed.captures == 1
    assert not graphed.overflowed()


def test_trajectory_matches_the_evaluation_kernels(cuda):
    S, T = 3, 10
    seq = _streams(61, 2048, T, S, cuda)
    net = _net(cuda)
    so = StreamingOdometry(net, streams=S, max_frames=T, graph=True)
    rows = []
    with torch.no_grad():
        so.step(seq[0])
        for k in range(1, T):
            rows.append(so.step(seq[k]).clone())
    rel, traj = so.relative_poses(), so.trajectory()
    assert rel.shape == traj.shape == (T, S, 4, 4) and rel.dtype == torch.float64
    eye = torch.eye(4, dtype=torch.float64, device=cuda).expand(S, 4, 4)
    assert torch.equal(rel[0], eye) and torch.equal(traj[0], eye)
    pose = torch.stack(rows)                                     # (T-1, S, 4, 7)
    ident = torch.tensor([0, 0, 0, 1, 0, 0, 0], dtype=torch.float32, device=cuda).expand(1, 4, 7)
    for i in range(S):
        mats = evaluation.rows_to_transforms(pose[:, i, 0, :])
        assert torch.equal(rel[1:, i], mats)                    # the same quat2mat body, bit for bit
        want = evaluation.compute_absolute_poses(torch.cat((eye[:1], mats)))
        assert torch.allclose(traj[:, i], want, rtol=1e-12, atol=1e-12)
        ev = evaluation.OdometryEvaluator(cuda)
        ev.add_batch([0] * T, list(range(T)), torch.cat((ident, pose[:, i])), torch.zeros(T, 4), torch.zeros(T, 3))
        ap, _ = ev.trajectories()[0]
        assert torch.allclose(traj[:, i], ap, rtol=1e-12, atol=1e-12)
    # full: the host refuses the next frame before the device would overflow
    with torch.no_grad(), pytest.raises(RuntimeError, match="max_frames=%d" % T):
        so.step(seq[0])
    assert so.frames_seen == T and not so.overflowed()
    assert so.frame_counts().tolist() == [T] * S
    so.reset()
    with torch.no_grad():
        assert so.step(seq[0]) is None
    assert so.relative_poses().shape == (1, S, 4, 4)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_reset_and_reprime_run_through_the_one_step(cuda, graph):
    """Lock step has no prime graph: the first frame and the first frame after reset() go through the same step (and in
    graph mode the same captured graph) as every pair; the state machine on the device primes all streams there."""
    S, T = 2, 3
    net = _net(cuda)
    fs = net._fused
    so = StreamingOdometry(net, streams=S, graph=graph)
    eye = torch.eye(4, dtype=torch.float64, device=cuda).expand(S, 4, 4)
    with torch.no_grad():
        for half, seed in enumerate((81, 85)):
            seq = _streams(seed, 1024, T, S, cuda)
            if half:
                so.reset()
            assert so.step(seq[0]) is None
            rows = []
            for k in range(1, T):
                got = so.step(seq[k]).clone()
                assert torch.equal(got, fs(_cm(seq[k - 1]), _cm(seq[k]))), (half, k)
                rows.append(got)
            pose = torch.stack(rows)                                 # (T-1, S, 4, 7)
            rel, traj = so.relative_poses(), so.trajectory()
            assert rel.shape == traj.shape == (T, S, 4, 4) and so.frames_seen == T
            assert torch.equal(rel[0], eye) and torch.equal(traj[0], eye)
            for i in range(S):
                mats = evaluation.rows_to_transforms(pose[:, i, 0, :])
                assert torch.equal(rel[1:, i], mats)
                want = evaluation.compute_absolute_poses(torch.cat((eye[:1], mats)))
                assert torch.allclose(traj[:, i], want, rtol=1e-12, atol=1e-12)
            assert so.frame_counts().tolist() == [T] * S
    if graph:
        assert so.captures == 1 and len(so._graphs) == 1
    assert not so.overflowed()


def test_posenet_odometry_at_the_real_size(cuda, tmp_path):
    """PWCLONetOdometry over 8 frames of 8192 points against the pair forward; checkpoint round trip through init()."""
    T = 8
    pcs = synthetic.kitti_like_sequence(5, 8192, T)[0]
    cfg = dict(device=str(cuda), num_input_channels=3, sequence_len=2, num_points=8192,
               posenet_config=dict(log_mode="none"))
    mod = PWCLONetPredictionModule(cfg)
    params.fill_state_dict(mod.pwclonet.state_dict())
    ckpt = str(tmp_path / "checkpoint.ckp")
    torch.save({"prediction_module": mod.state_dict()}, ckpt)

    def run(odo):
        odo.init()
        for k in range(T):
            data = {"numpy_pc": pcs[k] if k % 2 else torch.from_numpy(pcs[k])}     # arrays and tensors
            odo.process_next_frame(data)
            assert data["odometry_pose"].shape == (4, 4)
            if k == 0:
                assert np.array_equal(data["odometry_pose"], np.eye(4, dtype=np.float32))
        return odo.get_relative_poses()

    direct = PWCLONetOdometry(mod, device=cuda)
    got = run(direct)
    assert got.shape == (T, 4, 4) and got.dtype == np.float32
    assert np.array_equal(got[0], np.eye(4, dtype=np.float32))
    assert len(direct.elapsed) == T and direct.get_elapsed() > 0
    assert (direct.relative_pose_key(), direct.pointcloud_key()) == ("odometry_pose", "odometry_pc")
    frames = torch.from_numpy(pcs).to(cuda)
    net = mod.pwclonet
    with torch.no_grad():      # one stream = the pair forward at batch 1 (the cost volume's variant follows the batch)
        pair = torch.cat([net(_cm(frames[k - 1:k]), None, _cm(frames[k:k + 1]), None)[0] for k in range(1, T)])
    want = evaluation.rows_to_transforms(pair[:, 0, :]).float().cpu().numpy()
    assert np.array_equal(got[1:], want)
    fresh = PWCLONetPredictionModule(cfg)                        # untrained weights: init() must load the checkpoint
    loaded = PWCLONetOdometry(fresh, checkpoint_path=ckpt, device=cuda)
    assert np.array_equal(run(loaded), got)
    assert np.array_equal(run(loaded), got)                      # init() again: a new sequence from frame 0


def test_stream_errors(cuda):
    net = _net(cuda)
    seq = _streams(81, 1024, 3, 2, cuda)
    so = StreamingOdometry(net, streams=2, graph=False)
    with pytest.raises(RuntimeError, match="no_grad"):
        so.step(seq[0])
    with torch.no_grad():
        with pytest.raises(ValueError, match="at least 3 channels"):
            so.step(seq[0, :, :, :2].contiguous())
        with pytest.raises(ValueError, match="float32"):
            so.step(seq[0].double())
        with pytest.raises(ValueError, match="2 streams"):
            so.step(seq[0, :1])
        assert so.step(seq[0]) is None                            # primed: 2 streams of 1024 points
        with pytest.raises(ValueError, match="num_points"):
            so.step(seq[1, :, :512].contiguous())
        with pytest.raises(ValueError, match="2 streams"):
            so.step(torch.cat((seq[1], seq[1][:1])))
        assert so.step(seq[1]).shape == (2, 4, 7)
    net.train()
    with torch.no_grad(), pytest.raises(RuntimeError, match="eval-mode"):
        so.step(seq[2])
    off = _net(cuda, fused="off")
    with torch.no_grad(), pytest.raises(RuntimeError, match='"off"'):
        StreamingOdometry(off, streams=2).step(seq[0])
    assert so.frames_seen == 2
