"""GPU tests of ``StreamingOdometry(map=...)``: the global map follows the step's clouds and the
chosen trajectory, is rebuilt when the pose graph is optimised, and changes no existing output."""
import functools

import numpy as np
import pytest
import torch

import global_map_model as M
import icp_mask_model as masked
from oracle import params
from pwclonet_pylidarslam_amd import synthetic
from pwclonet_pylidarslam_amd.odometry import StreamingOdometry
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet

pytestmark = pytest.mark.gpu
S, N, FRAMES, V = 2, masked.N, 6, 0.5


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


@functools.lru_cache(maxsize=None)
def _seqs():
    return [synthetic.kitti_like_sequence(31 + i, N, FRAMES)[0] for i in range(S)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(gm, s, want, what):
    assert int(gm.totals()[s]) == want[2], (what, int(gm.totals()[s]), want[2])
    assert np.array_equal(gm.sources(s).cpu().numpy(), want[1]), what
    assert np.array_equal(_bits(gm.points(s).cpu().numpy()), _bits(want[0])), what


def test_lock_step_map_follows_the_optimised_trajectory(cuda):
    seqs, net = _seqs(), _net(cuda)
    kw = dict(streams=S, max_frames=8, backend=dict(source="network", max_loops=8, iters=6),
              loop=dict(min_id_distance=2, max_keyframes=8, verify=None))
    plain = StreamingOdometry(net, **kw)
    mapped = StreamingOdometry(net, map=dict(voxel_size=V, max_keyframes=8), **kw)
    assert mapped._map_source == "optimized"
    with torch.no_grad():
        for f in range(FRAMES):
            frames = torch.from_numpy(np.stack([seqs[s][f] for s in range(S)])).to(cuda)
            a, b = plain.step(frames), mapped.step(frames)
            assert (a is None and b is None) or torch.equal(a, b)
            gm = mapped.global_map()
            assert gm.counts().tolist() == [f + 1] * S and gm.built().tolist() == [f + 1] * S
            X = mapped.optimized_trajectory().cpu().numpy()
            for s in range(S):
                clouds = np.stack([seqs[s][k][:N, :3] for k in range(f + 1)])
                _same(gm, s, M.build(clouds, X[:, s], V, capacity=gm.capacity), (f, s))
    for name in ("relative_poses", "trajectory", "optimized_trajectory"):
        assert torch.equal(getattr(plain, name)(), getattr(mapped, name)()), name
    assert mapped.captures == plain.captures and gm.captures == 1 and not gm.overflowed() and plain.global_map() is None
    assert torch.equal(mapped.map_points(1), gm.points(1)) and gm.map_bytes() > 0

    # a loop edge moves the vertices: the map is rebuilt at them
    before = mapped.optimized_trajectory().clone()
    T = np.eye(4)
    T[:3, 3] = 0.4, -0.2, 0.1
    for s in range(S):
        mapped.backend().add_loop(s, 0, FRAMES - 1, T)
    mapped.backend().optimize()
    mapped.poll_loops(optimize=True)
    X = mapped.optimized_trajectory().cpu().numpy()
    assert not torch.equal(before, mapped.optimized_trajectory())
    for s in range(S):
        clouds = np.stack([seqs[s][k][:N, :3] for k in range(FRAMES)])
        want = M.build(clouds, X[:, s], V, capacity=gm.capacity)
        assert not np.array_equal(want[0], M.build(clouds, before.cpu().numpy()[:, s], V)[0])    # the edit moves the map
        _same(gm, s, want, ("rebuilt", s))
    assert gm.captures == 2
    mapped.poll_loops(optimize=True)                                             # nothing new: no further rebuild
    assert gm.calls == FRAMES + 1
    mapped.reset()
    assert gm.counts().tolist() == [0] * S and gm.totals().tolist() == [0] * S


def test_per_stream_map_with_a_dropout_and_a_restart(cuda):
    seqs, net = _seqs(), _net(cuda)
    active = np.array([[1, 1], [1, 1], [1, 0], [1, 1], [1, 1], [1, 1]], dtype=np.int32)
    restart = np.zeros_like(active)
    restart[4, 0] = 1
    plain = StreamingOdometry(net, streams=S, max_frames=8, per_stream=True)
    mapped = StreamingOdometry(net, streams=S, max_frames=8, per_stream=True, map=dict(voxel_size=V, max_keyframes=8, stride=2))
    assert mapped._map_source == "network"
    banks = [M.Bank(N, 8, stride=2) for _ in range(S)]
    delivered = [0] * S
    with torch.no_grad():
        for c in range(FRAMES):
            frames = np.full((S, N, 4), np.nan, dtype=np.float32)
            for s in range(S):
                if active[c, s]:
                    frames[s] = seqs[s][delivered[s]]
            frames = torch.from_numpy(frames).to(cuda)
            act, rst = active[c].tolist(), torch.from_numpy(restart[c]).to(cuda)
            a, b = plain.step(frames, active=act, restart=rst), mapped.step(frames, active=act, restart=rst)
            assert torch.equal(a, b) and torch.equal(plain.frame_counts(), mapped.frame_counts())
            counts = mapped.frame_counts().tolist()
            gm = mapped.global_map()
            for s in range(S):
                if active[c, s]:
                    primed = bool(restart[c, s]) or delivered[s] == 0
                    banks[s].advance(seqs[s][delivered[s]][:N, :3], counts[s] - 1, restart=primed)
                    delivered[s] += 1
                X = mapped.trajectory(stream=s).cpu().numpy()
                _same(gm, s, banks[s].map(X, V, gm.capacity), (c, s))
                assert int(gm.counts()[s]) == len(banks[s].frames), (c, s)
                for name in ("relative_poses", "trajectory"):
                    assert torch.equal(getattr(plain, name)(stream=s), getattr(mapped, name)(stream=s)), (c, s, name)
    assert mapped.frame_counts().tolist() == [2, 5] and gm.counts().tolist() == [1, 3]
    assert mapped.captures == plain.captures == 1 and gm.captures == 1
