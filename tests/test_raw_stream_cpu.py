"""CPU tests of streaming odometry from raw LiDAR sweeps: every host-side refusal of the raw mode is raised before any device
work, the new filter + compaction launcher is declared with the arity the binding uses, and the synthetic raw sweeps are
unfiltered, variable-length and deterministic."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from pwclonet_pylidarslam_amd import _lib, preprocess, synthetic
from pwclonet_pylidarslam_amd.odometry import PWCLONetOdometry, StreamingOdometry
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VELO_TO_CAM = [[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0], [1.0, 0.0, 0.0, 0.0]]


def _cpu_net():
    return PWCLONet(dict(num_input_channels=3, sequence_len=2, device="cpu", scalar_last=False, log_mode="none")).eval()


def _raw(net, S=2, capacity=4096, **kw):
    cfg = dict(dataset="kitti360", capacity=capacity)
    cfg.update(kw)
    return StreamingOdometry(net, streams=S, graph=False, sweeps=cfg)


def test_raw_mode_configuration_is_refused_on_the_host():
    net = _cpu_net()
    with pytest.raises(ValueError, match="tr"):
        _raw(net, dataset="kitti")                                          # KITTI needs its calibration
    with pytest.raises(ValueError, match="dataset"):
        _raw(net, dataset="nuscenes")
    with pytest.raises(ValueError, match="capacity"):
        _raw(net, capacity=0)
    with pytest.raises(ValueError, match="index limit"):
        _raw(net, S=1, capacity=preprocess.SWEEP_CAPACITY_LIMIT)            # at the sampler's index limit
    # streams x sampler workgroups beyond one plain launch: 131072 points = 8 workgroups per cloud, 24 clouds per launch
    assert preprocess.sampler_max_clouds(131072) == 24
    assert preprocess.sampler_max_clouds(24576) is None                     # register-resident sampler: no limit
    _raw(net, S=24, capacity=131072)
    with pytest.raises(ValueError, match="co-resident"):
        _raw(net, S=25, capacity=131072)
    with pytest.raises(ValueError, match="tr"):
        _raw(net, S=3, dataset="kitti", tr=np.zeros((2, 3, 4)))            # one calibration per stream, or one for all
    so = _raw(net, S=3, dataset="kitti", tr=VELO_TO_CAM)
    assert so.num_points == 8192 and so.survivor_counts() is None
    with pytest.raises(ValueError, match="tr"):
        so.set_calibration(np.zeros((3, 2)))
    so.set_calibration(np.stack([np.eye(4)[:3]] * 3))                       # host copy only: nothing allocated yet
    with pytest.raises(ValueError, match="calibration"):
        _raw(net, S=1).set_calibration(VELO_TO_CAM)                          # KITTI-360 has none


def test_step_sweeps_refusals_come_before_any_device_work():
    net = _cpu_net()
    so = _raw(net, S=2, capacity=4096)
    good = torch.zeros(2, 3000, 4)
    bad = [(good.double(), [10, 10], "float32"), (torch.zeros(2, 3000, 3), [10, 10], "4 channels"),
           (torch.zeros(3000, 4), [10], "float32"), (torch.zeros(3, 3000, 4), [10, 10, 10], "2 streams"),
           (torch.zeros(2, 5000, 4), [10, 10], "capacity=4096"), (good, [0, 10], "lengths"),
           (good, [10, 3001], "lengths"), (good, [10], "lengths"), (good, [1.5, 10], "lengths")]
    with torch.no_grad():
        for sweeps, lengths, msg in bad:
            with pytest.raises(ValueError, match=msg):
                so.step_sweeps(sweeps, lengths)
        with pytest.raises(RuntimeError, match="CPU not supported"):
            so.step_sweeps(good, [3000, 1])                                 # well formed, but on the host
        with pytest.raises(RuntimeError, match="CPU not supported"):
            so.step_sweeps(good, torch.tensor([3000, 1], dtype=torch.int32))
    so.frames_seen = so.max_frames                                          # full: refused first
    with torch.no_grad(), pytest.raises(RuntimeError, match="max_frames"):
        so.step_sweeps(good, [3000, 1])
    assert so.survivor_counts() is None and net._fused is None             # nothing allocated, nothing packed
    plain = StreamingOdometry(net, streams=2, graph=False)
    with torch.no_grad(), pytest.raises(RuntimeError, match="sweeps="):
        plain.step_sweeps(good, [3000, 1])


def test_posenet_odometry_raw_mode_refuses_host_sweeps():
    odo = PWCLONetOdometry(dict(num_input_channels=3, sequence_len=2, num_points=64), device="cpu",
                           sweeps=dict(dataset="kitti360", capacity=2048))
    odo.init()
    data = {"numpy_pc": np.zeros((1500, 4), dtype=np.float32)}
    with pytest.raises(RuntimeError, match="CPU not supported"):
        odo.process_next_frame(data)
    assert "odometry_pose" not in data
    with pytest.raises(ValueError, match="capacity"):
        odo.process_next_frame({"numpy_pc": np.zeros((3000, 4), dtype=np.float32)})
    with pytest.raises(ValueError, match="4 channels"):
        odo.process_next_frame({"numpy_pc": np.zeros((100, 3), dtype=np.float32)})
    assert odo.get_relative_poses().shape == (0, 4, 4)


def test_sweep_launcher_is_declared_with_the_header_arity():
    args, res = _lib.SIGNATURES["sweep_filter_compact_kernel_wrapper"]
    assert res is None
    with open(os.path.join(ROOT, "include", "pwclo_ops.h")) as f:
        header = f.read()
    m = re.search(r"void\s+sweep_filter_compact_kernel_wrapper\s*\(([^)]*)\)\s*;", header)
    assert m is not None, "sweep_filter_compact_kernel_wrapper is not declared in include/pwclo_ops.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(args) == len(params) == 11
    for p, a in zip(params, args):                              # pointers as c_void_p, floats as c_float, ints as c_int
        want = _lib._F if "*" in p else ctypes.c_float if p.startswith("float") else _lib._i
        assert a is want, (p, a)


def test_raw_sweep_sequence_is_unfiltered_variable_length_and_deterministic():
    sweeps, q, t = synthetic.raw_sweep_sequence(7, 4, n_azimuth=512)
    assert len(sweeps) == 4 and q.shape == (3, 4) and t.shape == (3, 3)
    lengths = [s.shape[0] for s in sweeps]
    assert len(set(lengths)) > 1                                            # the row count varies sweep by sweep
    for s in sweeps:
        assert s.dtype == np.float32 and s.ndim == 2 and s.shape[1] == 4 and s.shape[0] <= 64 * 512
        assert np.isfinite(s).all()
        assert (s[:, 3] >= 0).all() and (s[:, 3] <= 1).all()               # intensity column
        # velodyne frame (z up), nothing filtered: ground hits and far points are still there
        assert s[:, 2].min() < -1.5
        assert (np.abs(s[:, 0]) >= 30).any() or (np.abs(s[:, 1]) >= 30).any()
    again, q2, t2 = synthetic.raw_sweep_sequence(7, 4, n_azimuth=512)
    assert all(np.array_equal(a, b) for a, b in zip(sweeps, again))
    assert np.array_equal(q, q2) and np.array_equal(t, t2)
    other = synthetic.raw_sweep_sequence(8, 4, n_azimuth=512)[0]
    assert not np.array_equal(other[0][:100], sweeps[0][:100])
    with pytest.raises(ValueError):
        synthetic.raw_sweep_sequence(7, 1)
