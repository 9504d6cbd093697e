"""``StreamingOdometry(..., refine=dict(kind="voxel_map", ...))`` on the GPU: the network's outputs
beside a run without ``refine``, the refined poses beside a stand-alone ``VoxelMapRefiner`` fed the same clouds, in lock
step and per stream, and the refined motion as de-skew prior."""
import numpy as np
import pytest
import torch

import icp_mask_model as masked
import icp_model as model
import keyframe_model as kf
import test_gpu_icp_masked as knn_masked
import test_gpu_keyframe as keyed
import test_gpu_projective_stream as streamed
from pwclonet_pylidarslam_amd import _lib, evaluation, synthetic, voxel_map
from pwclonet_pylidarslam_amd.odometry import StreamingOdometry

pytestmark = pytest.mark.gpu

MAP = dict(voxel_size=2.0, extent=(32, 32, 8), iters=4, max_dist=2.0)
CFG = dict(MAP, kind="voxel_map")


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def test_lock_step_stream_beside_a_run_without_refine(cuda):
    S, n, frames = 2, 1024, 4
    seqs = [synthetic.kitti_like_sequence(31 + i, n, frames)[0] for i in range(S)]
    net = knn_masked._net(cuda)
    plain = StreamingOdometry(net, streams=S, graph=True)
    refined = StreamingOdometry(net, streams=S, graph=True, refine=dict(CFG, keyframe=dict(trans=0.05, rot=0.1)))
    alone = voxel_map.VoxelMapRefiner(S, n, graph=False, keyframe=dict(trans=0.05, rot=0.1), **MAP)
    eye = torch.eye(4, dtype=torch.float64, device=cuda).expand(S, 4, 4).contiguous()
    with torch.no_grad():
        for k in range(frames):
            frames_k = torch.from_numpy(np.stack([seqs[s][k] for s in range(S)])).to(cuda)
            a, b = plain.step(frames_k), refined.step(frames_k)
            assert (a is None) == (b is None) == (k == 0) and (a is None or torch.equal(a, b))
            guess = eye if b is None else evaluation.rows_to_transforms(b[:, 0, :].contiguous())
            T = alone.register(frames_k[:, :, :3].contiguous(), guess.contiguous())
            got = refined.refined_relative_poses()
            assert got.shape == (k + 1, S, 4, 4) and _same(got[k], eye if k == 0 else T), k
            assert torch.equal(refined.refiner().bufs["grid"], alone.bufs["grid"])
            if k:
                assert not (refined.refiner().status() & (model.FEW_PAIRS | model.BAD_PIVOT)).any()
    assert torch.equal(plain.relative_poses(), refined.relative_poses())
    assert torch.equal(plain.trajectory(), refined.trajectory())
    assert isinstance(refined.refiner(), voxel_map.VoxelMapRefiner) and refined.refiner().calls == frames
    assert refined.captures == plain.captures == 1 and refined.refiner()._graph is not None
    assert float(refined.refined_relative_poses()[1, :, :3, 3].norm(dim=-1).min()) > 0.3   # the registration found the motion
    _lib.synchronize(cuda)


def test_per_stream_stream_beside_lock_step_refiners(cuda):
    S, n = masked.S, masked.N
    seqs = [synthetic.kitti_like_sequence(31 + i, n, masked.CALLS)[0] for i in range(S)]
    net = knn_masked._net(cuda)
    plain = StreamingOdometry(net, streams=S, graph=True, per_stream=True)
    refined = StreamingOdometry(net, streams=S, graph=True, per_stream=True, refine=dict(CFG, per_stream=True))
    singles = [voxel_map.VoxelMapRefiner(1, n, graph=False, **MAP) for _ in range(S)]
    rows = [[] for _ in range(S)]
    with torch.no_grad():
        for c, call in enumerate(masked.schedule()):
            for so in (plain, refined):
                if call["reset"]:
                    so.reset(streams=call["reset"])
            frames = np.full((S, n, seqs[0].shape[2]), np.nan, dtype=np.float32)
            for s in range(S):
                if call["active"][s]:
                    frames[s] = seqs[s][call["frame"][s]]
            frames = torch.from_numpy(frames).to(cuda)
            act, rst = call["active"].tolist(), torch.from_numpy(call["restart"]).to(cuda)
            a, b = plain.step(frames, active=act, restart=rst), refined.step(frames, active=act, restart=rst)
            assert torch.equal(a, b) and torch.equal(plain.valid(), refined.valid())
            valid, status = refined.valid().tolist(), refined.refiner().status().tolist()
            for s in range(S):
                assert torch.equal(plain.relative_poses(stream=s), refined.relative_poses(stream=s))
                assert torch.equal(plain.trajectory(stream=s), refined.trajectory(stream=s))
                if not call["active"][s]:
                    assert status[s] == masked.IDLE
                    continue
                if not valid[s]:
                    rows[s] = []
                    assert status[s] == model.FEW_PAIRS
                rows[s].append(knn_masked._follow(singles[s], frames[s, :, :3], b[s:s + 1, 0, :], not valid[s]))
                got = refined.refined_relative_poses(stream=s)
                assert got.shape == (len(rows[s]), 4, 4) and _same(got, torch.stack(rows[s])), (c, s)
    assert refined.frame_counts().tolist() == [5, 1, 3]
    assert refined.captures == plain.captures == 1 and refined.refiner().calls == masked.CALLS
    _lib.synchronize(cuda)


def test_feedback_hands_the_refined_motion_to_the_deskew_prior(cuda):
    cfg = dict(CFG, iters=2)
    bare, bare_poses, bare_motions, _ = keyed._stream(cuda, None, deskew=True)
    off, off_poses, off_motions, _ = keyed._stream(cuda, dict(cfg), deskew=True)
    assert keyed._equal_poses(bare_poses, off_poses)
    for a, b in zip(bare_motions, off_motions):                                 # no feedback: the network's rows, bit for bit
        assert keyed._same(a, b)
    on, poses, motions, refined = keyed._stream(cuda, dict(cfg, feedback=True), deskew=True)
    moved = 0
    for k in range(1, streamed.FRAMES):
        T, got = refined[k].cpu().numpy(), motions[k].cpu().numpy()
        for s in range(streamed.S):
            assert keyed._ulps(got[s], kf.pose_row(T[s])).max() <= 1, (k, s)      # within one fp32 step of the model's row
        moved += int(not keyed._same(motions[k], poses[k][:, 0, :].contiguous()))
    assert moved > 0 and on.captures == 1 and isinstance(on.refiner(), voxel_map.VoxelMapRefiner)
    _lib.synchronize(cuda)
