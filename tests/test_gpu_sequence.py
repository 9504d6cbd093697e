"""Sequence odometry (``PWCLONet.forward_sequence``): every frame's pyramid runs once, the T - 1 consecutive pairs
share it.  The bar is the pair path itself: for the same pairs, poses, every neighbour list and the pyramid taps are
bit-identical to the fused pair forward (any env switch, fp32 and bf16 packing), through graph replay and the
windowed pipeline too."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import params
from pwclonet_pylidarslam_amd import evaluation, synthetic
from pwclonet_pylidarslam_amd.graphed import GraphedSequence, PipelinedSequence
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _net(dev, dtype=None, log_mode="none", fused="auto"):
    net = PWCLONet(dict(num_input_channels=3, sequence_len=2, device=str(dev), scalar_last=False, log_mode=log_mode,
                        fused=fused))
    params.fill_state_dict(net.state_dict())
    net = net.to(dev).eval()
    if fused != "off":
        net.prepare_fused(dtype=dtype)
    return net


def _frames(seed, n, t, dev):
    pcs, q, tr = synthetic.kitti_like_sequence(seed, n, t)
    return torch.from_numpy(pcs).to(dev), q, tr


def _cm(frames):
    """(B, N, c) point-major frames -> the pair forward's (B, 3, N) input."""
    return frames[:, :, :3].permute(0, 2, 1).contiguous()


def _pairs(frames):
    """(frames[:-1], frames[1:]) as the pair forward's inputs."""
    return _cm(frames[:-1]), _cm(frames[1:])


def _pose_close(pose, ref, what):
    pose, ref = pose.detach().cpu().double(), ref.detach().cpu().double()
    err, scale = (pose - ref).abs().max().item(), ref.abs().max().item()
    print("\n%s: max |pose - ref| = %.3e, max |ref| = %.3f" % (what, err, scale))
    assert err <= 1e-5 * scale + 1e-6, "%s: |pose - ref| = %.3e exceeds 1e-5 * %.3f + 1e-6" % (what, err, scale)


SWITCHES = [("default", {}, None), ("hoist0", {"PWCLO_HOIST": "0"}, None), ("knn_reuse0", {"PWCLO_KNN_REUSE": "0"}, None),
            ("early_cv0", {"PWCLO_EARLY_CV": "0"}, None), ("pw_tail0", {"PWCLO_PW_TAIL": "0"}, None),
            ("head_warp0", {"PWCLO_HEAD_WARP": "0"}, None), ("bf16", {}, "bf16")]


@pytest.mark.parametrize("name,env,dtype", SWITCHES, ids=[s[0] for s in SWITCHES])
def test_sequence_is_bitwise_the_pair_forward(cuda, monkeypatch, name, env, dtype):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    frames, _, _ = _frames(3, 4096, 9, cuda)                     # (9, 4096, 4): c = 4 goes through the ingest kernel
    net = _net(cuda, dtype)
    assert net._fused.hoist == (env.get("PWCLO_HOIST", "1") == "1")
    x1, x2 = _pairs(frames)
    with torch.no_grad():
        pose_pair, inter_pair = net._fused(x1, x2, return_intermediates=True)
        pose_seq, inter_seq = net._fused.forward_sequence(frames, 4096, return_intermediates=True)
        api, log = net.forward_sequence(frames)
        api_pair, _ = net(x1, None, x2, None)
    assert pose_seq.shape == (8, 4, 7)
    assert torch.equal(pose_seq, pose_pair)
    assert torch.equal(api, api_pair) and torch.equal(api, pose_seq)
    assert log == {}                                             # log_mode "none", as the pair forward
    assert sorted(inter_seq["lists"]) == sorted(inter_pair["lists"])
    P = frames.shape[0] - 1
    for key, idx in inter_pair["lists"].items():
        got = inter_seq["lists"][key]
        if key.startswith("psa_"):          # pyramid lists: pair mode holds 2P clouds, sequence mode each frame once
            assert got.shape[0] == P + 1 and idx.shape[0] == 2 * P, key
            assert torch.equal(got[:P], idx[:P]) and torch.equal(got[1:], idx[P:]), key
        else:                               # pair-stage lists: one per pair on both sides
            assert torch.equal(got, idx), key
    for key in ("x11", "f13", "flow", "emb1", "mask1"):
        assert torch.equal(inter_seq[key], inter_pair[key]), key


def test_sequence_at_the_bench_shape(cuda):
    """33 frames x 8192 points (one window of the sequence tool) against pair batch 32 (bench.py's batch)."""
    frames, _, _ = _frames(5, 8192, 33, cuda)
    clouds = frames[:, :, :3].contiguous()                       # contiguous (T, N, 3): used without an ingest launch
    net = _net(cuda)
    x1, x2 = _pairs(frames)
    with torch.no_grad():
        pair, _ = net(x1, None, x2, None)
        seq, _ = net.forward_sequence(clouds)
        seq4, _ = net.forward_sequence(frames, 8192)
    assert seq.shape == (32, 4, 7)
    assert torch.equal(seq, pair) and torch.equal(seq4, pair)


@pytest.mark.parametrize("case", ["n1024_b2", "n8192_b1"])
def test_two_frame_windows_match_the_reference_golden(cuda, case):
    z = np.load(os.path.join(GOLDEN, "pwclonet_%s.npz" % case))
    meta = json.loads(str(z["meta"]))
    if meta["generator"] == "uniform":
        pc1, pc2 = synthetic.uniform_pair(meta["seed"], meta["npoints"], meta["batch"])
    else:
        pc1, pc2, _, _ = synthetic.kitti_like_pair(meta["seed"], meta["npoints"], meta["batch"])
    net = _net(cuda)
    ref = torch.from_numpy(z["pose_params"])
    for b in range(meta["batch"]):
        window = torch.from_numpy(np.stack((pc1[b], pc2[b]))).to(cuda)
        with torch.no_grad():
            pose, _ = net.forward_sequence(window)
        _pose_close(pose[0], ref[b], "T=2 window %s[%d] vs reference golden" % (case, b))


def test_graph_replay_and_windowed_pipeline(cuda):
    """A replayed window is the eager window; the windowed pipeline (depth 2, n = 23, window 9) is one-shot
    ``forward_sequence`` on all 23 frames.  8 and 22 pairs run the same pair-stage kernel variants at these cloud
    sizes (the cost volume's first aggregate is chosen by the launch size)."""
    net = _net(cuda)
    a, _, _ = _frames(7, 4096, 23, cuda)
    b, _, _ = _frames(8, 4096, 23, cuda)
    with torch.no_grad():
        ref_a = net.forward_sequence(a)[0].clone()
        ref_b = net.forward_sequence(b)[0].clone()
        eager = net.forward_sequence(a[:9])[0].clone()
    g = GraphedSequence(net)
    assert torch.equal(g(a[:9]), eager)
    assert torch.equal(g(a[:9]), eager)                          # replay, not the capture run
    # windows of 9 frames at 0, 8 and 14 (the tail moved back to full length, its first two rows come from the second)
    pipe = PipelinedSequence(net, window=9, depth=2)
    outs = [pipe(a), pipe(b), pipe(a), pipe(b)]                  # two sequences alternated over two slots
    torch.cuda.synchronize(cuda)
    for got, ref in zip(outs, [ref_a, ref_b, ref_a, ref_b]):
        assert got.shape == (22, 4, 7)
        assert torch.equal(got, ref)
    tail = pipe(a[:13])                                          # windows (0, 9) and (4, 9): the tail overlaps by 5
    assert torch.equal(tail, ref_a[:12])


def test_raw_frames_to_bf16_sequence(cuda):
    """configs[4] shape: raw 120k-row frames -> filter -> compaction -> exact sampling -> bf16 sequence forward.  Three
    frames = one sampler launch of 3 x 8 workgroups (the large-cloud residency rule allows 16 frames per launch)."""
    import bench
    from pwclonet_pylidarslam_amd import preprocess
    net = _net(cuda, "bf16")
    raw = bench.raw_frames(21, 3, 120000, cuda)
    clouds, counts = preprocess.frames_to_clouds(raw, 8192, "kitti360", near_threshold=35.0)
    assert int(counts.min()) > 24576                              # the multi-workgroup sampler's range
    x1, x2 = _pairs(clouds)
    with torch.no_grad():
        seq, _ = net.forward_sequence(clouds)
        pair, _ = net(x1, None, x2, None)
    assert torch.equal(seq, pair)


def test_sequence_rows_feed_the_evaluator(cuda):
    """The reference's evaluation rows: frame 0 prepended once (pairs (0,0), (0,1), ...), frame_ids = second frame."""
    frames, q, t = _frames(9, 2048, 24, cuda)
    n = frames.shape[0]
    gq = torch.from_numpy(np.concatenate(([[1.0, 0.0, 0.0, 0.0]], q)).astype(np.float32)).to(cuda)
    gt = torch.from_numpy(np.concatenate(([[0.0, 0.0, 0.0]], t)).astype(np.float32)).to(cuda)
    net = _net(cuda)
    with torch.no_grad():
        rows, _ = net.forward_sequence(torch.cat((frames[:1], frames)))
    assert rows.shape == (n, 4, 7)
    ev_seq = evaluation.OdometryEvaluator(cuda, segments=(5, 10), step_size=2)
    ev_seq.add_batch([4] * n, list(range(n)), rows, gq, gt)
    ev_pair = evaluation.OdometryEvaluator(cuda, segments=(5, 10), step_size=2)
    prev = torch.cat((frames[:1], frames[:-1]))
    for s in range(0, n, 8):                                      # pair batches of 8, as a dataset loop would feed them
        with torch.no_grad():
            pose, _ = net(_cm(prev[s:s + 8]), None, _cm(frames[s:s + 8]), None)
        ev_pair.add_batch([4] * pose.shape[0], list(range(s, s + pose.shape[0])), pose, gq[s:s + 8], gt[s:s + 8])
    (ap, ag), (bp, bg) = ev_seq.trajectories()[4], ev_pair.trajectories()[4]
    assert torch.equal(ap, bp) and torch.equal(ag, bg)
    rs, rp = ev_seq.evaluate()[4], ev_pair.evaluate()[4]
    assert rs["ave_t_err"] is not None
    assert torch.equal(rs["seq_err"], rp["seq_err"])
    assert (rs["ave_t_err"], rs["ave_r_err"], rs["segment"]) == (rp["ave_t_err"], rp["ave_r_err"], rp["segment"])


def test_sequence_validation_errors(cuda):
    from pwclonet_pylidarslam_amd.prediction import PWCLONetPredictionModule
    net = _net(cuda)
    frames, _, _ = _frames(11, 1024, 3, cuda)
    with torch.no_grad():
        with pytest.raises(ValueError, match="at least 2 frames"):
            net.forward_sequence(frames[:1])
        with pytest.raises(ValueError, match="at least 3 channels"):
            net.forward_sequence(frames[:, :, :2].contiguous())
        with pytest.raises(ValueError, match="num_points"):
            net.forward_sequence(frames, 2048)
    with pytest.raises(RuntimeError, match="no_grad"):
        net.forward_sequence(frames)
    net.train()
    with torch.no_grad(), pytest.raises(RuntimeError, match="eval-mode"):
        net.forward_sequence(frames)
    off = _net(cuda, fused="off")
    with torch.no_grad(), pytest.raises(RuntimeError, match='"off"'):
        off.forward_sequence(frames)
    # the adapter: num_points from its config
    mod = PWCLONetPredictionModule(dict(device=str(cuda), num_input_channels=3, sequence_len=2, num_points=1024,
                                        posenet_config=dict(log_mode="none")))
    params.fill_state_dict(mod.pwclonet.state_dict())
    mod = mod.to(cuda).eval()
    with torch.no_grad():
        got, _ = mod.forward_sequence(frames)
        ref, _ = mod.pwclonet.forward_sequence(frames[:, :1024])
    assert torch.equal(got, ref)
