"""Per-stream streaming odometry, the parts that need no GPU: the state machine model of
tests/stream_mask_model.py over its schedule, the two sections of the kept neighbour-search workspace as the built library
reports them, the declarations of the new launchers, and the host-side refusals of ``per_stream=True``."""
import ctypes
import os
import re

import pytest
import torch

import stream_mask_model as model
from pwclonet_pylidarslam_amd import _lib
from pwclonet_pylidarslam_amd.odometry import StreamingOdometry
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I, R, P = model.IDLE, model.PRIME, model.PAIR


def test_state_machine_model_over_the_schedule():
    m = model.StreamMaskModel(4, 64)
    kinds, counts, pairs = [], [], []
    for active, restart in model.SCHEDULE:
        out = m.step(active, restart)
        kinds.append([k for k, _, _ in out])
        counts.append(list(m.count))
        pairs.append([prev for _, _, prev in out])
        assert m.valid == [int(k == P) for k, _, _ in out]
    assert kinds == [[R, I, I, I],            # stream 0's first frame; 1-3 idle before theirs
                     [P, R, I, I],
                     [P, I, R, R],            # stream 1's gap begins
                     [P, I, P, P],            # restart of the idle stream 1: ignored
                     [P, P, R, P],            # stream 1 is back and pairs; stream 2 restarts with a frame
                     [R, P, P, R],            # two restarts in one call
                     [I, P, P, P],
                     [P, P, P, P]]
    assert counts == [[1, 0, 0, 0], [2, 1, 0, 0], [3, 1, 1, 1], [4, 1, 2, 2], [5, 2, 1, 3], [1, 3, 2, 1], [1, 4, 3, 2],
                      [2, 5, 4, 3]]
    assert pairs[4][1] == 1                   # after the gap: paired with the frame delivered before it (call 1)
    assert pairs[7][0] == 5                   # after idling: paired with the frame that primed (call 5)
    assert m.have_prev == [1, 1, 1, 1] and m.overflow == 0 and m.calls == len(model.SCHEDULE)


def test_state_machine_model_refuses_a_full_trajectory():
    m = model.StreamMaskModel(1, 2)
    assert m.step([1], [0]) == [(R, 0, None)]
    assert m.step([1], [0]) == [(P, 1, 0)]
    assert m.step([1], [0]) == [(P, None, 1)]          # full: nothing written
    assert m.count == [2] and m.overflow == 1
    assert m.step([1], [1]) == [(R, 0, None)] and m.count == [1]


def test_workspace_sections_tile_the_workspace():
    lib = _lib.load()
    out = (ctypes.c_longlong * 4)()
    for b, n in ((1, 256), (2, 1000), (3, 1024), (5, 2048), (32, 8192), (7, 16384)):
        total = lib.knn_point_workspace_bytes(b, n)
        assert total > 0
        assert lib.knn_point_workspace_sections(b, n, out) == 1
        rows_off, rows_bytes, boxes_off, boxes_bytes = list(out)
        assert rows_off == 0 and rows_bytes > 0 and boxes_bytes > 0
        assert rows_off + b * rows_bytes == boxes_off
        assert boxes_off + b * boxes_bytes == total
        assert rows_bytes % 16 == 0 and boxes_bytes % 16 == 0           # every cloud's piece moves 16 bytes per lane
    for b, n in ((2, 64), (2, 255), (1, 16385)):                        # exhaustive-kernel sizes: no workspace
        assert lib.knn_point_workspace_bytes(b, n) == 0
        out[:] = [9, 9, 9, 9]
        assert lib.knn_point_workspace_sections(b, n, out) == 0
        assert list(out) == [0, 0, 0, 0]


@pytest.mark.parametrize("name,arity,ret", [("stream_append_masked_kernel_wrapper", 11, "void"),
                                            ("stream_handover_masked_kernel_wrapper", 8, "void"),
                                            ("knn_point_workspace_sections", 3, "int")])
def test_new_launchers_are_declared_exported_and_bound_alike(name, arity, ret):
    args, res = _lib.SIGNATURES[name]
    assert res is (None if ret == "void" else ctypes.c_int)
    with open(os.path.join(ROOT, "include", "pwclo_ops.h")) as f:
        header = f.read()
    m = re.search(r"%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), header)
    assert m is not None, "%s is not declared in include/pwclo_ops.h" % name
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(args) == len(params) == arity
    for p, a in zip(params, args):                                      # pointers never travel as c_int
        assert (a is _lib._i) == ("*" not in p), (p, a)
    assert hasattr(_lib.load(), name)                                   # the built library exports it
    assert "int pwclo_abi_version(void);" in header and _lib.load().pwclo_abi_version() == 1


def _cpu_net():
    return PWCLONet(dict(num_input_channels=3, sequence_len=2, device="cpu", scalar_last=False, log_mode="none")).eval()


def test_per_stream_host_side_refusals():
    net = _cpu_net()
    lock = StreamingOdometry(net, streams=2, graph=False)
    assert lock.per_stream is False
    with torch.no_grad(), pytest.raises(ValueError, match="per_stream=True"):
        lock.step(torch.zeros(2, 64, 3), active=[1, 0])
    with pytest.raises(ValueError, match="per_stream=True"):
        lock.reset(streams=[0])
    with pytest.raises(ValueError, match="per_stream=True"):
        lock.relative_poses(stream=0)
    so = StreamingOdometry(net, streams=3, max_frames=4, graph=False, per_stream=True)
    assert so.per_stream and so.valid() is None and so.frame_counts() is None
    for accessor in (so.relative_poses, so.trajectory):
        with pytest.raises(ValueError, match="stream=i"):
            accessor()
        assert accessor(stream=1).shape == (0, 4, 4)
        with pytest.raises(ValueError, match="outside"):
            accessor(stream=3)
    assert so._stream_mask([True, False, True], "active").tolist() == [1, 0, 1]
    assert so._stream_mask([0, 2, 0], "active").tolist() == [0, 1, 0]
    assert so._stream_mask([2, 0]).tolist() == [1, 0, 1]                # reset(streams=[...]): a list of indices
    assert so._stream_mask([False, True, False]).tolist() == [0, 1, 0]
    for bad in ([1, 0], [1.0, 0.0, 1.0], [[1, 0, 1]]):
        with pytest.raises(ValueError, match="active"):
            so._stream_mask(bad, "active")
    with pytest.raises(ValueError, match="outside"):
        so.reset(streams=[3])
    so.reset(streams=[1])                                               # nothing on the device yet: no launch, no error
    so.frames_seen = 4                                                  # max_frames bounds the calls since a full reset
    with torch.no_grad(), pytest.raises(RuntimeError, match="max_frames=4"):
        so.step(torch.zeros(3, 64, 3))
    so.reset()
    assert so.frames_seen == 0
    with torch.no_grad(), pytest.raises(RuntimeError, match="CPU not supported"):
        so.step(torch.zeros(3, 64, 3), active=[1, 1, 0])
