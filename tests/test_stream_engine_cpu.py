"""``stream_engine``, the parts that need no GPU: the call counter of an eager ``Replay`` and the
argument vocabulary, whose messages are compared with literal copies of the texts the modules raised before they shared it."""
import numpy as np
import pytest
import torch

from pwclonet_pylidarslam_amd import stream_engine as E


def _message(fn, *args, **kw):
    """-> (exception type, message) of a call that must raise."""
    with pytest.raises((ValueError, RuntimeError)) as e:
        fn(*args, **kw)
    return e.type, str(e.value)


def test_eager_replay_counts_calls_and_never_touches_the_device(monkeypatch):
    def forbidden(*a, **kw):
        raise AssertionError("an eager Replay reached for torch.cuda")
    for name in ("synchronize", "CUDAGraph", "graph"):
        monkeypatch.setattr(torch.cuda, name, forbidden)
    r, seen = E.Replay(False), []
    for k in range(4):
        r.run(lambda: seen.append(k), None, key=k % 2)
        assert r.calls == k + 1 and r.captures == 0 and r.graphs == {} and r.graph(k % 2) is None and r.graph() is None
    assert seen == [0, 1, 2, 3]
    r.drop()
    assert r.calls == 4 and r.captures == 0

    def body():
        raise KeyError("the body's own")
    with pytest.raises(KeyError):
        r.run(body, None)
    assert r.calls == 4 and r.captures == 0 and r.graphs == {}

    class Owner(E.Replayed):
        replay = r
    assert Owner().calls == 4 and Owner().captures == 0
    with pytest.raises(AttributeError):
        Owner().calls = 0                               # read-only


def test_need_raises_in_order_with_the_texts_of_before():
    f32, strided = torch.zeros(2, 3), torch.zeros(2, 6)[:, ::2]
    # kind and shape come first, whatever else is wrong with the tensor
    assert _message(E.need, f32, "solve: T", torch.float64, (2, 3)) == (
        ValueError, "solve: T must be a float64 tensor of shape (2, 3), got torch.float32 (2, 3)")
    assert _message(E.need, strided, "op: x", torch.float32, (2, 4)) == (
        ValueError, "op: x must be a float32 tensor of shape (2, 4), got torch.float32 (2, 3)")
    assert _message(E.need, f32, "normals: xyz", torch.int32) == (
        ValueError, "normals: xyz must be a int32 tensor, got torch.float32 (2, 3)")
    assert _message(E.need, [1.0], "op: x", torch.float32, (1,)) == (
        ValueError, "op: x must be a float32 tensor of shape (1,), got <class 'list'> ()")
    # then where it lives: a host tensor that is not contiguous either is refused for the device
    assert _message(E.need, strided, "op: x", torch.float32, (2, 3)) == (RuntimeError, "CPU not supported")
    assert _message(E.need, f32, "op: x", torch.float32) == (RuntimeError, "CPU not supported")
    # cuda=False leaves that question to the caller: the layout is next
    assert _message(E.need, strided, "GlobalMap: cloud", torch.float32, (2, 3), cuda=False) == (
        ValueError, "GlobalMap: cloud must be contiguous")
    assert E.need(f32, "op: x", torch.float32, (2, 3), cuda=False) is None
    assert E.need(f32, "op: x", torch.float32, cuda=False) is None
    assert _message(E.need_cuda, None, f32) == (RuntimeError, "CPU not supported")
    assert E.need_cuda(None, None) is None and E.ptr(None) == 0 and E.ptr(f32) == f32.data_ptr()


def test_stream_index_and_indices():
    assert [E.stream_index("GlobalMap", "points", s, 2) for s in (0, 1, np.int64(1))] == [0, 1, 1]
    for s in (-1, 2):                                   # a stream of -1 and a stream equal to S
        assert _message(E.stream_index, "GlobalMap", "points", s, 2) == (
            ValueError, "GlobalMap: points: stream=%d outside [0, 2)" % s)
        assert _message(E.stream_indices, "GlobalMap", "reset", [0, s], 2) == (
            ValueError, "GlobalMap: reset: stream=%d outside [0, 2)" % s)
    assert _message(E.stream_index, "ScanContextLoopDetector", "database", 3, 3) == (
        ValueError, "ScanContextLoopDetector: database: stream=3 outside [0, 3)")
    assert _message(E.stream_index, None, "add_loop", 2, 2) == (ValueError, "add_loop: stream=2 outside [0, 2)")
    assert _message(E.stream_index, "VoxelMapRefiner", None, -1, 2) == (ValueError, "VoxelMapRefiner: stream=-1 outside [0, 2)")
    assert list(E.stream_indices("GlobalMap", "reset", None, 3)) == [0, 1, 2]
    assert E.stream_indices("GlobalMap", "reset", [2, 0, 2], 3) == [2, 0, 2] and E.stream_indices(None, "reset", [], 3) == []
    assert E.stream_count("PoseGraph", 1024, 1024) == 1024 and E.stream_count("PoseGraph", np.int32(1), 1024) == 1
    for S in (0, 1025):
        assert _message(E.stream_count, "PoseGraph", S, 1024) == (ValueError, "PoseGraph: streams=%d outside [1, 1024]" % S)


def test_frame_ids():
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    given, ids = E.frame_ids("GlobalMap", [3, 0], 2)
    assert given is None and ids.dtype == torch.int32 and ids.tolist() == [3, 0]
    given, ids = E.frame_ids("GlobalMap", np.array([7, 8], dtype=np.uint8), 2)
    assert given is None and ids.dtype == torch.int32 and ids.tolist() == [7, 8]
    t = i32(4, 5)
    given, ids = E.frame_ids("GlobalMap", t, 2)
    assert given is t and ids is t                      # a tensor is the caller's: where it lives is asked later
    text = "ScanContextLoopDetector: frame_ids must be (2,) non-negative integers"
    for bad in ([0], [0, -1], [0.5, 1.0], [0.0, 1.0], [[0, 1]]):          # wrong shape, negative id, float dtype
        assert _message(E.frame_ids, "ScanContextLoopDetector", bad, 2) == (ValueError, text)
    assert _message(E.frame_ids, "GlobalMap", torch.zeros(2, dtype=torch.int64), 2) == (
        ValueError, "GlobalMap: frame_ids must be a int32 tensor of shape (2,), got torch.int64 (2,)")
    assert _message(E.frame_ids, "GlobalMap", torch.tensor([0, 1]), 2)[0] is ValueError
    assert _message(E.frame_ids, "GlobalMap", i32(0, 1, 2), 2) == (
        ValueError, "GlobalMap: frame_ids must be a int32 tensor of shape (2,), got torch.int32 (3,)")
    assert _message(E.frame_ids, "GlobalMap", torch.zeros(2), 2) == (
        ValueError, "GlobalMap: frame_ids must be a int32 tensor of shape (2,), got torch.float32 (2,)")
    assert _message(E.frame_ids, "GlobalMap", i32(0, 1, 2, 3)[::2], 2) == (ValueError, "GlobalMap: frame_ids must be contiguous")


def test_pose_stack():
    poses = torch.eye(4, dtype=torch.float64).expand(5, 2, 4, 4).contiguous()
    assert E.pose_stack("GlobalMap", "poses", poses, 2) is None and E.pose_stack("GlobalMap", "poses", poses[:1], 2) is None
    text = "GlobalMap: rebuild: poses must be float64 (frames >= 1, 2, 4, 4)"
    for bad in (poses[0], poses[:0], poses.numpy(), None):               # not a stack, no frame, not a tensor
        assert _message(E.pose_stack, "GlobalMap: rebuild", "poses", bad, 2) == (ValueError, text)
    assert _message(E.pose_stack, "GlobalMap", "poses", poses.float(), 2) == (
        ValueError, "GlobalMap: poses must be a float64 tensor of shape (5, 2, 4, 4), got torch.float32 (5, 2, 4, 4)")
    assert _message(E.pose_stack, "GlobalMap", "poses", poses[:, :1], 2) == (
        ValueError, "GlobalMap: poses must be a float64 tensor of shape (5, 2, 4, 4), got torch.float64 (5, 1, 4, 4)")
    what = "ScanContextLoopDetector"
    assert _message(E.pose_stack, what, "trajectory", torch.zeros(3, 2, 4, 4), 2) == (
        ValueError, what + ": trajectory must be a float64 tensor of shape (3, 2, 4, 4), got torch.float32 (3, 2, 4, 4)")
    assert _message(E.pose_stack, what, "trajectory", torch.zeros(0, 2, 4, 4, dtype=torch.float64), 2) == (
        ValueError, what + ": trajectory must be float64 (frames >= 1, 2, 4, 4)")
    assert _message(E.pose_stack, what, "trajectory", torch.zeros(3, 2, 4, 8, dtype=torch.float64)[..., :4], 2) == (
        ValueError, what + ": trajectory must be contiguous")


def test_init_poses_and_the_solver_settings():
    ok64, ok32 = torch.zeros(2, 4, 4, dtype=torch.float64), torch.zeros(2, 7)
    assert E.init_poses("IcpRefiner", ok64, 2) is None and E.init_poses("IcpRefiner", ok32, 2) is None
    head = "IcpRefiner: init must be float64 (2, 4, 4) or float32 (2, 7) pose rows, got "
    assert _message(E.init_poses, "IcpRefiner", ok64.float(), 2) == (ValueError, head + "torch.float32 (2, 4, 4)")
    assert _message(E.init_poses, "IcpRefiner", ok32.double(), 2) == (ValueError, head + "torch.float64 (2, 7)")
    assert _message(E.init_poses, "IcpRefiner", ok64[:1], 2) == (ValueError, head + "torch.float64 (1, 4, 4)")
    assert _message(E.init_poses, "IcpRefiner", None, 2) == (ValueError, head + "<class 'NoneType'> ()")
    w = "ProjectiveIcpRefiner"
    assert _message(E.need_iters, w, 0) == (ValueError, w + ": iters=0 must be >= 1")
    assert _message(E.need_sigma, w, 0.0) == (ValueError, w + ": sigma=0.0 must be finite and > 0")
    assert _message(E.need_sigma, w, float("inf")) == (ValueError, w + ": sigma=inf must be finite and > 0")
    assert _message(E.need_max_dist, w, -1) == (ValueError, w + ": max_dist=-1 must be >= 0")
    assert _message(E.need_max_dist, w, float("nan")) == (ValueError, w + ": max_dist=nan must be >= 0")
    assert _message(E.need_solver, w, -1e-6, 1e-4, 64) == (ValueError, w + ": damping=-1e-06 must be finite and >= 0")
    assert _message(E.need_solver, w, 1e-6, -1.0, 64) == (ValueError, w + ": threshold_delta_pose=-1.0 must be >= 0")
    assert _message(E.need_solver, w, 1e-6, 1e-4, 0) == (
        ValueError, w + ": min_pairs=0 must be >= 1 (an empty map freezes a stream through it)")
    assert _message(E.need_solver, w, -1.0, -1.0, 0)[1] == w + ": damping=-1.0 must be finite and >= 0"     # in this order
    assert E.need_iters(w, 1) is None and E.need_sigma(w, 0.5) is None and E.need_max_dist(w, 0) is None
    assert E.need_solver(w, 0.0, 0.0, 1) is None
