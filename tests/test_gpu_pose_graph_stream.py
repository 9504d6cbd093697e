"""GPU tests of the reference-shaped facade over the device pose graph."""
import numpy as np
import pytest
import torch

import functools

import icp_mask_model as masked
import pose_graph_cases as pgc
import pose_graph_device as pgd
from oracle import params
from pwclonet_pylidarslam_amd import synthetic
from pwclonet_pylidarslam_amd.odometry import StreamingOdometry
from pwclonet_pylidarslam_amd.pose_graph import PoseGraph
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _net(dev):
    """The suite's synthetic weights with every pose head's last layer set to "no motion" (tests/test_gpu_icp_masked.py)."""
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


REFINE = dict(kind="knn", map_size=2, iters=8, max_dist=2.0)
BACKEND = dict(max_loops=4, max_absolute=2, iters=6)


def test_backend_arguments():
    net = object()
    with pytest.raises(ValueError, match="refine"):
        StreamingOdometry(net, backend=dict(source="refined"))
    with pytest.raises(ValueError, match="source"):
        StreamingOdometry(net, backend=dict(source="icp"))
    with pytest.raises(ValueError, match="max_poses"):
        StreamingOdometry(net, backend=dict(source="network", max_poses=7))
    with pytest.raises(RuntimeError, match="backend"):
        StreamingOdometry(net).optimized_trajectory()


@pytest.mark.parametrize("source", ["refined", "network"])
def test_lock_step_backend_keeps_every_output_and_optimises(cuda, source):
    S, n, F = 2, masked.N, 6
    seqs = [synthetic.kitti_like_sequence(31 + i, n, F)[0] for i in range(S)]
    net = _net(cuda)
    plain = StreamingOdometry(net, streams=S, max_frames=8, refine=dict(REFINE))
    backed = StreamingOdometry(net, streams=S, max_frames=8, refine=dict(REFINE), backend=dict(BACKEND, source=source))
    with torch.no_grad():
        for f in range(F):
            frames = torch.from_numpy(np.stack([seqs[s][f] for s in range(S)])).to(cuda)
            a, b = plain.step(frames), backed.step(frames)
            assert (a is None and b is None) or torch.equal(a, b)
    for name in ("relative_poses", "trajectory", "refined_relative_poses", "refined_trajectory"):
        assert torch.equal(getattr(plain, name)(), getattr(backed, name)()), name
    assert plain.captures == backed.captures == 1 and not backed.backend().overflowed()
    pg = backed.backend()
    chain = backed.refined_relative_poses() if source == "refined" else backed.relative_poses()
    assert pg.counts().tolist() == [F] * S and torch.equal(pg.relative_poses(), chain)
    assert torch.equal(backed.optimized_trajectory(), backed.refined_trajectory() if source == "refined" else backed.trajectory())
    # one loop on stream 1, optimised, against a stand-alone graph given the same edges
    Z = pgc.pgm.pose([0, 0, 1], 0.02, [0.3, 0.1, 0.0])
    before = backed.optimized_trajectory().clone()
    pg.add_loop(1, 0, F - 1, Z)
    pg.optimize()
    alone = PoseGraph(S, max_poses=8, **BACKEND)
    for k in range(1, F):
        alone.append(chain[k].contiguous())
    alone.add_loop(1, 0, F - 1, Z)
    alone.optimize()
    got = backed.optimized_trajectory()
    assert torch.equal(got, alone.poses()) and torch.equal(got[:, 0], before[:, 0]) and not torch.equal(got[:, 1], before[:, 1])
    rel = backed.optimized_relative_poses().cpu().numpy()
    X = got.cpu().numpy()
    assert np.array_equal(rel[0], np.tile(np.eye(4), (S, 1, 1))) and np.abs(X[2] @ rel[3] - X[3]).max() <= 1e-12
    for name in ("trajectory", "refined_trajectory"):                 # the optimisation touches no other output
        assert torch.equal(getattr(plain, name)(), getattr(backed, name)()), name


def test_per_stream_schedule_matches_one_graph_per_stream(cuda):
    """The six-call schedule of dropouts and a restart (tests/test_gpu_icp_masked.py): every stream's graph holds what a
    graph of its own holds when it is fed that stream's refined poses alone."""
    S, n = masked.S, masked.N
    seqs = [synthetic.kitti_like_sequence(31 + i, n, masked.CALLS)[0] for i in range(S)]
    net = _net(cuda)
    cfg = dict(REFINE, per_stream=True)
    plain = StreamingOdometry(net, streams=S, max_frames=8, per_stream=True, refine=dict(cfg))
    backed = StreamingOdometry(net, streams=S, max_frames=8, per_stream=True, refine=dict(cfg), backend=dict(BACKEND))
    singles = [PoseGraph(1, max_poses=8, **BACKEND) for _ in range(S)]
    with torch.no_grad():
        for c, call in enumerate(masked.schedule()):
            for so in (plain, backed):
                if call["reset"]:
                    so.reset(streams=call["reset"])
            frames = np.full((S, n, seqs[0].shape[2]), np.nan, dtype=np.float32)
            for s in range(S):
                if call["active"][s]:
                    frames[s] = seqs[s][call["frame"][s]]
            frames = torch.from_numpy(frames).to(cuda)
            act, rst = call["active"].tolist(), torch.from_numpy(call["restart"]).to(cuda)
            a, b = plain.step(frames, active=act, restart=rst), backed.step(frames, active=act, restart=rst)
            assert torch.equal(a, b) and torch.equal(plain.frame_counts(), backed.frame_counts())
            valid = backed.valid().tolist()
            for s in range(S):
                if not call["active"][s]:
                    continue
                if valid[s]:
                    singles[s].append(backed.refined_relative_poses(stream=s)[-1][None].contiguous())
                else:
                    singles[s].reset()
                for name in ("relative_poses", "trajectory", "refined_relative_poses", "refined_trajectory"):
                    assert torch.equal(getattr(plain, name)(stream=s), getattr(backed, name)(stream=s)), (c, s, name)
            pg = backed.backend()
            started = backed.frame_counts() > 0                       # (a stream that never delivered holds vertex 0 alone)
            assert torch.equal(pg.counts()[started], backed.frame_counts()[started])
            for s in range(S):
                if int(pg.counts()[s]) >= 1 and backed.frame_counts()[s] > 0:
                    assert torch.equal(backed.optimized_trajectory(stream=s), singles[s].poses(0)), (c, s)
                    assert torch.equal(pg.relative_poses(s), backed.refined_relative_poses(stream=s)), (c, s)
    assert backed.frame_counts().tolist() == [5, 1, 3] and backed.captures == 1 and not pg.overflowed()
    Z = pgc.pgm.pose([0, 0, 1], 0.01, [0.2, 0.0, 0.0])
    pg.add_loop(0, 0, 4, Z); singles[0].add_loop(0, 0, 4, Z)
    with pytest.raises(ValueError):
        pg.add_loop(1, 0, 1, Z)                                       # stream 1 restarted: one pose
    pg.optimize(); singles[0].optimize()
    assert torch.equal(backed.optimized_trajectory(stream=0), singles[0].poses(0))
    assert torch.equal(backed.optimized_trajectory(stream=2), singles[2].poses(0))


def test_graph_slam_facade_on_the_circle():
    from pwclonet_pylidarslam_amd.backend import GraphSLAM, GraphSLAMConfig
    g, _ = pgc.circle(N=128)
    slam = GraphSLAM(GraphSLAMConfig(max_poses=128, max_loops=8, max_absolute=8, max_optim_iterations=20))
    slam.init()
    assert slam.need_to_synchronise_poses() is False
    for k in range(1, g.n):
        frame = {GraphSLAM.se3_odometry_constraint(k - 1): (g.Z[k], None), "numpy_pc_0": np.zeros((4, 3))}
        if k == g.n - 1:
            i, j, Z, Om = g.loops[0]
            frame[GraphSLAM.se3_loop_closure_constraint(i, j)] = (Z, Om)
        slam.next_frame(frame)
        if k < g.n - 1:
            assert slam.need_to_synchronise_poses() is False           # a chain-only frame
    assert slam.need_to_synchronise_poses() is True and slam.need_to_synchronise_poses() is False
    assert len(slam.registered_odometry_constraints()) == 100 and len(slam.registered_loop_constraints()) == 1
    assert slam.registered_absolute_constraints() == []
    pg = pgd.make([g], iters=20)
    pg.optimize()
    direct = pg.poses(0).cpu().numpy()
    assert np.array_equal(slam.world_poses(), direct) and slam.absolute_poses().shape == (101, 4, 4)
    rel = slam.relative_odometry_poses()
    assert np.array_equal(rel[0], np.eye(4)) and np.allclose(direct[4] @ rel[5], direct[5], atol=1e-12)
    assert np.linalg.norm(direct[100, :3, 3]) < 1e-3


def test_graph_slam_offline_restarts_from_the_odometry():
    from pwclonet_pylidarslam_amd.backend import GraphSLAM, GraphSLAMConfig
    g, gt = pgc.noisy_chain(20, 71, N=32)
    slam = GraphSLAM(GraphSLAMConfig(max_poses=32, max_loops=4, max_absolute=4, max_optim_iterations=10,
                                     online_optimization=False))
    slam.init()
    for k in range(1, g.n):
        frame = {GraphSLAM.se3_odometry_constraint(k - 1): (g.Z[k], None)}
        if k in (12, 19):
            frame[GraphSLAM.se3_loop_closure_constraint(0, k)] = (pgc.between(gt, 0, k), None)
        slam.next_frame(frame)
    g.add_loop(0, 12, pgc.between(gt, 0, 12)); g.add_loop(0, 19, pgc.between(gt, 0, 19))
    pg = pgd.make([g], iters=10)                                      # both loops, one optimisation from the odometry
    pg.optimize()
    assert np.array_equal(slam.world_poses(), pg.poses(0).cpu().numpy())
    assert GraphSLAM._regexes()[1] == "^se3_loop_closure_constraint_([\\d]+)_([\\d]+)$"
