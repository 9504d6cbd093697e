"""CPU tests of streaming odometry's host side: argument checks, the refusal of host tensors by every entry point, the
``max_frames`` bookkeeping before anything reaches a device, and the trajectory launcher's declaration."""
import os
import re

import numpy as np
import pytest
import torch

from pwclonet_pylidarslam_amd import _lib
from pwclonet_pylidarslam_amd.odometry import MAX_STREAMS, PWCLONetOdometry, StreamingOdometry
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cpu_net():
    return PWCLONet(dict(num_input_channels=3, sequence_len=2, device="cpu", scalar_last=False, log_mode="none")).eval()


def test_stream_entry_points_refuse_host_tensors():
    net = _cpu_net()
    frames = torch.zeros(1, 64, 3)
    for graph in (False, True):
        so = StreamingOdometry(net, streams=1, graph=graph)
        with torch.no_grad(), pytest.raises(RuntimeError, match="CPU not supported"):
            so.step(frames)
        assert so.frames_seen == 0 and so.relative_poses().shape == (0, 1, 4, 4)
    odo = PWCLONetOdometry(dict(num_input_channels=3, sequence_len=2, num_points=64), device="cpu")
    odo.init()
    data = {"numpy_pc": np.zeros((64, 4), dtype=np.float32)}
    with pytest.raises(RuntimeError, match="CPU not supported"):
        odo.process_next_frame(data)
    assert "odometry_pose" not in data
    assert odo.get_relative_poses().shape == (0, 4, 4)
    assert net._fused is None                                    # nothing was packed for a refused call


def test_stream_arguments_and_max_frames_bookkeeping():
    net = _cpu_net()
    for bad in (dict(streams=0), dict(streams=MAX_STREAMS + 1), dict(max_frames=0), dict(num_points=0)):
        with pytest.raises(ValueError):
            StreamingOdometry(net, **bad)
    so = StreamingOdometry(net, streams=3, max_frames=5, num_points=32, graph=False)
    assert (so.streams, so.max_frames, so.num_points, so.frames_seen) == (3, 5, 32, 0)
    # the capacity check comes first and needs no device: a full stream refuses the next frame before any launch
    so.frames_seen = 5
    with torch.no_grad(), pytest.raises(RuntimeError, match="max_frames=5"):
        so.step(torch.zeros(3, 64, 3))
    so.reset()
    assert so.frames_seen == 0
    with torch.no_grad(), pytest.raises(RuntimeError, match="CPU not supported"):
        so.step(torch.zeros(3, 64, 3))                            # room again: the frame itself is refused


def test_stream_launcher_is_declared_with_the_header_arity():
    args, res = _lib.SIGNATURES["stream_append_masked_kernel_wrapper"]
    assert res is None
    with open(os.path.join(ROOT, "include", "pwclo_ops.h")) as f:
        header = f.read()
    m = re.search(r"void\s+stream_append_masked_kernel_wrapper\s*\(([^)]*)\)\s*;", header)
    assert m is not None, "stream_append_masked_kernel_wrapper is not declared in include/pwclo_ops.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(args) == len(params) == 11
    for p, a in zip(params, args):                              # pointers travel as c_void_p, ints as c_int
        assert (a is _lib._F) == ("*" in p), (p, a)


def test_the_lock_step_launcher_is_gone_and_lock_step_refuses_the_per_stream_arguments():
    with open(os.path.join(ROOT, "include", "pwclo_ops.h")) as f:
        assert "odom_stream_append_kernel_wrapper" not in f.read()
    assert "odom_stream_append_kernel_wrapper" not in _lib.SIGNATURES
    lock = StreamingOdometry(_cpu_net(), streams=2, graph=False)
    frames = torch.zeros(2, 64, 3)
    masks = "StreamingOdometry: active / restart masks need per_stream=True"
    with torch.no_grad():                                        # refused before the frames are looked at
        with pytest.raises(ValueError, match=re.escape(masks)):
            lock.step(frames, active=[1, 0])
        with pytest.raises(ValueError, match=re.escape(masks)):
            lock.step(frames, restart=[0, 1])
    raw = StreamingOdometry(_cpu_net(), streams=2, graph=False, sweeps=dict(dataset="kitti360", capacity=64))
    for kw in (dict(active=[1, 0]), dict(restart=[0, 1])):
        with torch.no_grad(), pytest.raises(ValueError, match=re.escape(masks)):
            raw.step_sweeps(torch.zeros(2, 64, 4), [64, 64], **kw)
    with pytest.raises(ValueError, match=re.escape("StreamingOdometry: reset(streams=...) needs per_stream=True")):
        lock.reset(streams=[0])
    for accessor in (lock.relative_poses, lock.trajectory):
        with pytest.raises(ValueError, match=re.escape("StreamingOdometry: stream= needs per_stream=True (lock-step "
                                                       "trajectories are (frames, S, 4, 4))")):
            accessor(stream=0)
    assert lock.frames_seen == 0 and lock.frame_counts() is None
