"""``StreamingOdometry(..., sweeps=..., refine=dict(kind="projective", ...))``: the network's rows stay
bit for bit those of a run without ``refine``, and the refined poses are those of a stand-alone ``ProjectiveIcpRefiner`` fed
the rows the sweep front end kept and the level-1 guesses."""
import functools

import numpy as np
import pytest
import torch

from oracle import params
from pwclonet_pylidarslam_amd import _lib, evaluation, projective, synthetic
from pwclonet_pylidarslam_amd.odometry import StreamingOdometry
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet

pytestmark = pytest.mark.gpu

CAP, ROWS, N, S, FRAMES = 16384, 12000, 1024, 2, 4
IMAGE = dict(height=8, width=64, up_fov=3.0, down_fov=-24.8)


@functools.lru_cache(maxsize=None)
def _net(dev):
    """The suite's synthetic weights with every pose head's last layer set to (q, t) = ((1, 0, 0, 0), 0), as in
    tests/test_gpu_icp.py: the untrained network's pose is no motion at all, a guess a registration can start from."""
    net = PWCLONet(dict(num_input_channels=3, sequence_len=2, device=str(dev), scalar_last=False, log_mode="none",
                        fused="auto"))
    sd = net.state_dict()
    params.fill_state_dict(sd)
    for key, v in sd.items():
        if key.endswith(("conv1d_q.conv.weight", "conv1d_t.conv.weight", "conv1d_t.conv.bias")):
            v.zero_()
        elif key.endswith("conv1d_q.conv.bias"):
            v.copy_(torch.tensor([1.0, 0.0, 0.0, 0.0]))
    net = net.to(dev).eval()
    net.prepare_fused()
    return net


@functools.lru_cache(maxsize=None)
def _batches(dev):
    seqs = [synthetic.raw_sweep_sequence(41 + s, FRAMES)[0] for s in range(S)]
    out = []
    for k in range(FRAMES):
        rows = [np.asarray(seqs[s][k])[s::10][:ROWS - 100 * s - 10 * k] for s in range(S)]    # every tenth row: the full circle
        batch = np.zeros((S, max(r.shape[0] for r in rows), 4), dtype=np.float32)
        for s, r in enumerate(rows):
            batch[s, :r.shape[0]] = r
        out.append((torch.from_numpy(batch).to(dev), [r.shape[0] for r in rows]))
    return out


def _run(dev, refine, sink=None):
    odo = StreamingOdometry(_net(dev), streams=S, num_points=N, graph=True, sweeps=dict(dataset="kitti360", capacity=CAP),
                            refine=refine)
    poses = []
    with torch.no_grad():
        for batch, lengths in _batches(dev):
            pose = odo.step_sweeps(batch, lengths)
            poses.append(None if pose is None else pose.clone())
            if sink is not None:
                b = odo.front.bufs
                sink.append((b["packed"].clone(), b["counts"].clone()))
    return odo, poses


def test_projective_refine_beside_a_run_without(cuda):
    cfg = dict(kind="projective", map_size=2, iters=4, min_pairs=16, max_dist=2.0, **IMAGE)
    plain, plain_poses = _run(cuda, None)
    kept = []
    refined, poses = _run(cuda, cfg, kept)
    for a, b in zip(plain_poses, poses):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))       # pose rows
    assert torch.equal(plain.relative_poses(), refined.relative_poses())
    assert torch.equal(plain.trajectory(), refined.trajectory())
    assert refined.captures == 1 and refined.refiner().captures == 1                 # one capture of each graph
    assert isinstance(refined.refiner(), projective.ProjectiveIcpRefiner) and refined.refiner().calls == FRAMES
    alone = projective.ProjectiveIcpRefiner(S, CAP, graph=False, **{k: v for k, v in cfg.items() if k != "kind"})
    ref = refined.refined_relative_poses()
    assert ref.shape == (FRAMES, S, 4, 4)
    eye = torch.eye(4, dtype=torch.float64, device=cuda).expand(S, 4, 4)
    acc = eye.clone()
    for k, (packed, counts) in enumerate(kept):
        assert int(counts.min()) > 64
        guess = eye if poses[k] is None else evaluation.rows_to_transforms(poses[k][:, 0, :].contiguous())
        T = alone.register(packed, counts, guess.contiguous())
        if k == 0:
            assert torch.equal(ref[0], eye)
        else:
            assert torch.equal(ref[k], T)                                            # the stand-alone refiner's bits
            assert int(alone.diagnostics()["pairs"].min()) >= 16
        acc = torch.matmul(acc, ref[k])
        assert (refined.refined_trajectory()[k] - acc).abs().max() < 1e-9
    _lib.synchronize(cuda)


def test_kind_rules_and_the_default(cuda):
    net = _net(cuda)
    sweeps = dict(dataset="kitti360", capacity=CAP)
    with pytest.raises(ValueError, match="sweeps"):
        StreamingOdometry(net, streams=S, refine=dict(kind="projective", **IMAGE))
    with pytest.raises(ValueError, match="lock step only"):
        StreamingOdometry(net, streams=S, sweeps=sweeps, per_stream=True, refine=dict(kind="projective", per_stream=True,
                                                                                     **IMAGE))
    cfg = dict(map_size=2, iters=2, max_dist=2.0)
    outs = []
    for extra in (dict(), dict(kind="knn")):                                         # no kind: bit for bit kind="knn"
        odo, poses = _run(cuda, dict(cfg, **extra))
        outs.append((odo.refined_relative_poses().clone(), odo.refined_trajectory().clone(), poses))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    for a, b in zip(outs[0][2], outs[1][2]):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
    _lib.synchronize(cuda)
