"""CPU tests of sequence odometry's host side: window / overlap / tail bookkeeping of the windowed pipeline, the
refusal of host tensors, the sequence generator (deterministic per seed, steps in ``kitti_like_pair``'s convention)
and the ingest launcher's declaration."""
import numpy as np
import pytest
import torch

from pwclonet_pylidarslam_amd import synthetic
from pwclonet_pylidarslam_amd.graphed import sequence_windows


@pytest.mark.parametrize("n,window", [(2, 2), (9, 9), (23, 9), (33, 33), (34, 33), (100, 33), (5, 2), (17, 4), (5, 9)])
def test_windows_cover_every_pair_once(n, window):
    wins = sequence_windows(n, window)
    assert wins[0][0] == 0 and wins[-1][0] + wins[-1][1] == n
    assert all(length == min(n, window) for _, length, _ in wins)     # full-length windows only (short sequence: one)
    for (s0, l0, _), (s1, _, f1) in zip(wins, wins[1:]):
        assert s1 + f1 == s0 + l0 - 1                            # consecutive windows share at least the boundary frame
    assert all(f == 0 for _, _, f in wins[:-1])
    pairs = [s + i for s, length, first in wins for i in range(first, length - 1)]
    assert pairs == list(range(n - 1))                           # every pair (i, i + 1) from exactly one window, in order


def test_window_tail_and_errors():
    assert sequence_windows(23, 9) == [(0, 9, 0), (8, 9, 0), (14, 9, 2)]
    assert sequence_windows(25, 9) == [(0, 9, 0), (8, 9, 0), (16, 9, 0)]
    assert sequence_windows(33, 33) == [(0, 33, 0)]
    assert sequence_windows(34, 33) == [(0, 33, 0), (1, 33, 31)]
    assert sequence_windows(5, 9) == [(0, 5, 0)]
    with pytest.raises(ValueError):
        sequence_windows(1, 9)
    with pytest.raises(ValueError):
        sequence_windows(9, 1)


def test_sequence_entry_points_refuse_host_tensors():
    from pwclonet_pylidarslam_amd.graphed import PipelinedSequence
    from pwclonet_pylidarslam_amd.prediction import PWCLONetPredictionModule
    from pwclonet_pylidarslam_amd.pwclonet import PWCLONet
    net = PWCLONet(dict(num_input_channels=3, sequence_len=2, device="cpu", scalar_last=False, log_mode="none")).eval()
    frames = torch.zeros(3, 64, 3)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="CPU not supported"):
            net.forward_sequence(frames)
        mod = PWCLONetPredictionModule(dict(device="cpu", num_input_channels=3, sequence_len=2, num_points=64)).eval()
        with pytest.raises(RuntimeError, match="CPU not supported"):
            mod.forward_sequence(frames)
        with pytest.raises(RuntimeError, match="CPU not supported"):
            PipelinedSequence(net, window=2, depth=1)(frames)
    assert net._fused is None                                    # nothing was packed for a refused call


def test_sequence_generator_is_deterministic_per_seed():
    a = synthetic.kitti_like_sequence(3, 1024, 5)
    b = synthetic.kitti_like_sequence(3, 1024, 5)
    c = synthetic.kitti_like_sequence(4, 1024, 5)
    for x, y in zip(a, b):
        assert x.dtype == np.float32 and np.array_equal(x, y)
    assert not np.array_equal(a[0], c[0])
    pcs, q, t = a
    assert pcs.shape == (5, 1024, 4) and q.shape == (4, 4) and t.shape == (4, 3)
    # the pair generators' streams are untouched by the new generator
    p1 = synthetic.kitti_like_pair(3, 1024, 1)
    synthetic.kitti_like_sequence(3, 1024, 3)
    assert all(np.array_equal(x, y) for x, y in zip(p1, synthetic.kitti_like_pair(3, 1024, 1)))
    with pytest.raises(ValueError):
        synthetic.kitti_like_sequence(3, 1024, 1)
    with pytest.raises(RuntimeError, match="usable points"):
        synthetic.kitti_like_sequence(3, 10 ** 6, 2)


def _rot(q):
    w, x, y, z = q.astype(np.float64)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _median_nn(a, b):
    d = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    return float(np.median(np.sqrt(d.min(axis=1))))


def test_sequence_generator_steps_follow_the_pair_convention():
    """Step i maps frame i + 1 into frame i (p_i = R(q_i) p_{i+1} + t_i, camera frame), as (q_gt, t_gt) of
    ``kitti_like_pair`` map its frame 2 into frame 1; the motion law is the pair's (|yaw| <= 2 deg, 0.5-1.5 m
    forward = camera z)."""
    pcs, q, t = synthetic.kitti_like_sequence(12, 2048, 6)
    yaw = 2 * np.arctan2(-q[:, 2], q[:, 0])
    assert np.allclose(np.linalg.norm(q, axis=1), 1.0, atol=1e-6)
    assert (np.abs(yaw) <= np.deg2rad(2.0) + 1e-6).all() and (q[:, [1, 3]] == 0).all()
    assert (t[:, :2] == 0).all() and (t[:, 2] >= 0.5).all() and (t[:, 2] <= 1.5).all()
    for i in range(5):
        a, b = pcs[i, :, :3].astype(np.float64), pcs[i + 1, :, :3].astype(np.float64)
        moved = b @ _rot(q[i]).T + t[i]
        aligned, raw = _median_nn(moved, a), _median_nn(b, a)
        assert aligned < 0.6 * raw, (i, aligned, raw)


def test_sequence_ingest_is_declared():
    from pwclonet_pylidarslam_amd import _lib
    args, res = _lib.SIGNATURES["ingest_sequence_kernel_wrapper"]
    assert len(args) == 6 and res is None
