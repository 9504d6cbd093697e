"""The global map, the parts that need no GPU: the NumPy model of tests/global_map_model.py against a
second, row-by-row implementation, the properties the design rests on (append, duplicates), the ABI's new names,
``global_map_bytes``, the host's refusals and the scene property that makes the map worth rebuilding."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import global_map_cases as C            # noqa: E402
import global_map_model as M            # noqa: E402
import loop_closure_cases as LC         # noqa: E402
from pwclonet_pylidarslam_amd import _lib, global_map       # noqa: E402
from pwclonet_pylidarslam_amd.odometry import StreamingOdometry     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the model ---------------------------------------------------------------------------------------------------------

def second_model(clouds, X, v, lengths=None, capacity=None):
    """The rule once more, one row at a time in Python scalars: a dictionary from key to the first row that has it."""
    K, n = clouds.shape[:2]
    seen, points, source = {}, [], []
    for k in range(K):
        T = [[float(X[k][a][b]) for b in range(4)] for a in range(3)]
        length = n if lengths is None else min(max(int(lengths[k]), 0), n)
        for i in range(length):
            x, y, z = (float(c) for c in clouds[k, i])
            with np.errstate(all="ignore"):
                w = [np.float32(np.float64(((T[a][0] * x + T[a][1] * y) + T[a][2] * z) + T[a][3])) for a in range(3)]
            q = []
            for a in range(3):
                d = float(w[a]) / float(v)
                if not abs(d) < 2147483648.0:               # NaN and infinities too
                    q = None
                    break
                q.append(round(d))                          # Python rounds halves to even, as rint does
            if q is None:
                continue
            h = (M.K0 * q[0] + M.K1 * q[1] + M.K2 * q[2]) & M.MASK
            if h not in seen:
                seen[h] = (k, i)
                points.append(w)
                source.append((k, i))
    total = len(points)
    if capacity is not None:
        points, source = points[:capacity], source[:capacity]
    return np.array(points, dtype=M.F).reshape(-1, 3), np.array(source, dtype=np.int32).reshape(-1, 2), total


def same(a, b):
    return a[2] == b[2] and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name, n, K, v", C.SMALL)
def test_model_agrees_with_the_row_by_row_dictionary(name, n, K, v):
    clouds, X, lengths = C.case(name, n, K, v)
    got = M.build(clouds, X, v, lengths=lengths)
    assert same(got, second_model(clouds, X, v, lengths))
    cap = max(1, got[2] // 2)
    assert same(M.build(clouds, X, v, lengths=lengths, capacity=cap), second_model(clouds, X, v, lengths, cap))


def test_families_hit_what_they_are_named_for():
    for v in C.VOXELS:
        assert M.build(*C.case("one_voxel", 65, 3, v)[:2], v)[2] == 1
        c, X, _ = C.case("same_cloud", 65, 3, v)
        p, src, total = M.build(c, X, v)
        assert total == M.build(c[:1], X[:1], v)[2] and (src[:, 0] == 0).all()
        c, X, _ = C.case("marker", 65, 3, v)
        _, src, _ = M.build(c, X, v)
        assert ((src[:, 0] == 0) & (src[:, 1] == 65 // 2)).sum() == 1           # the marker voxel's first row wins, once
        assert not ((src[:, 1] == 64)).any()
        c, X, _ = C.case("far_pose", 65, 1, v)
        assert M.build(c, X, v)[2] == 0
        c, X, _ = C.case("bad_pose", 65, 1, v)
        assert M.build(c, X, v)[2] == 0
        c, X, lengths = C.case("partial", 65, 3, v)
        _, src, _ = M.build(c, X, v, lengths=lengths)
        assert (src[:, 1] < lengths[src[:, 0]]).all() and not (src[:, 0] == 1).any()
    c, X, _ = C.case("halfway", 65, 3, 0.5)
    w = M.world(c[0], X[0]).astype(np.float64) / 0.5
    assert np.array_equal(w - np.floor(w), np.full_like(w, 0.5))               # exactly between two voxels


@pytest.mark.parametrize("name", ["uniform", "dense", "shifted", "non_finite", "partial"])
def test_adding_keyframes_only_appends(name):
    clouds, X, lengths = C.case(name, 65, 40, 0.3)
    prev = M.build(clouds[:1], X, 0.3, lengths=None if lengths is None else lengths[:1])
    for k in range(2, 41):
        cur = M.build(clouds[:k], X, 0.3, lengths=None if lengths is None else lengths[:k])
        m = prev[2]
        assert cur[2] >= m and np.array_equal(cur[0][:m].view(np.uint32), prev[0].view(np.uint32))
        assert np.array_equal(cur[1][:m], prev[1])
        prev = cur


def test_a_duplicate_keyframe_adds_nothing():
    clouds, X, _ = C.case("uniform", 257, 3, 0.3)
    base = M.build(clouds, X, 0.3)
    twice = M.build(np.concatenate([clouds, clouds[1:2]]), X, 0.3, frames=[0, 1, 2, 1])
    assert same(base, twice)


def test_bank_follows_stride_capacity_and_max_new():
    b = M.Bank(4, max_keyframes=3, stride=2, max_new=1)
    for f in range(7):
        b.advance(np.zeros((4, 3)), f)
    assert b.frames == [0, 2, 4] and b.overflow and b.built == 3
    b = M.Bank(4, max_keyframes=8, stride=1, max_new=2)
    b.clouds, b.frames, b.lengths = [np.zeros((4, 3))] * 3, [0, 1, 2], [4] * 3
    b.advance(np.zeros((4, 3)), 3)
    assert b.built == 2
    b.advance(np.zeros((4, 3)), 5, restart=True)
    assert b.frames == [5] and b.built == 1


# ---- the scene property ------------------------------------------------------------------------------------------------

def test_the_map_at_the_true_path_is_smaller_than_at_the_drifted_chain():
    r = LC.revisit()
    frames = r["frames"][:, 0]
    assert frames.shape == (40, 1024, 3)
    path = np.stack(r["path"])
    true = np.linalg.inv(path[0]) @ path
    chain = [np.eye(4)]
    for k in range(1, 40):
        chain.append(chain[-1] @ r["chain"][k])
    chain = np.stack(chain)
    at_true, at_chain = M.build(frames, true, 0.3)[2], M.build(frames, chain, 0.3)[2]
    assert (at_true, at_chain) == (5875, 8285)
    assert at_true <= 0.8 * at_chain
    assert (M.build(frames, true, 0.1)[2], M.build(frames, chain, 0.1)[2]) == (14246, 28978)


# ---- declarations ------------------------------------------------------------------------------------------------------

NEW = [("global_map_begin_kernel_wrapper", 14), ("global_map_push_kernel_wrapper", 6), ("global_map_clear_kernel_wrapper", 6),
       ("global_map_insert_kernel_wrapper", 14), ("global_map_count_kernel_wrapper", 10),
       ("global_map_scan_kernel_wrapper", 5), ("global_map_write_kernel_wrapper", 17), ("global_map_end_kernel_wrapper", 2)]


def _header():
    with open(os.path.join(ROOT, "include", "pwclo_ops.h")) as f:
        return f.read()


@pytest.mark.parametrize("name, arity", NEW)
def test_new_symbols_are_declared_with_the_header_arity(name, arity):
    args, res = _lib.SIGNATURES[name]
    m = re.search(r"void\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m is not None, "%s is not declared in include/pwclo_ops.h" % name
    assert res is None
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(args) == len(params) == arity
    for p, a in zip(params, args):
        want = _lib._F if "*" in p else ctypes.c_float if p.startswith("float") else \
            ctypes.c_double if p.startswith("double") else _lib._i
        assert a is want, (name, p, a)
    assert hasattr(_lib.load(), name)


def test_global_map_bytes_and_the_version():
    lib = _lib.load()
    header = _header()
    names = {n for n, _ in NEW} | {"global_map_bytes"}
    assert set(re.findall(r"\b(global_map_\w+)\s*\(", header)) == names
    assert {n for n in _lib.SIGNATURES if n.startswith("global_map_")} == names
    assert "12. global map" in header
    assert _lib.SIGNATURES["global_map_bytes"] == ([_lib._i] * 4, ctypes.c_longlong)
    assert lib.pwclo_abi_version() == 1                                          # additions only
    for S, MK, n, cap in ((1, 1024, 8192, 1 << 22), (8, 1024, 8192, 1 << 22), (3, 5, 96, 480), (1, 1, 1, 1), (2, 40, 1024, 7),
                          (1, 65535, 8192, 100), (1024, 1, 31, 31)):
        T = global_map.table_slots(MK, n)
        assert T >= 64 and T >= 2 * MK * n and (T == 64 or T < 4 * MK * n) and T & (T - 1) == 0
        want = S * (8 * T + 4 * (T + 2) + 16 * MK * n + 8 * MK + 4 * MK * ((n + 255) // 256) + 32 + 20 * cap)
        assert lib.global_map_bytes(S, MK, n, cap) == want == global_map.map_bytes(S, MK, n, cap)
    one = global_map.map_bytes(1, 1024, 8192, 1 << 22)                          # the figure DESIGN.md section 27 states
    assert one - 20 * (1 << 22) - 8 - 8 * 1024 - 4 * 1024 * 32 - 32 == 12 * (1 << 24) + 16 * (1 << 23) == 335544320
    for bad in ((0, 4, 4, 1), (1025, 4, 4, 1), (1, 0, 4, 1), (1, 65536, 4, 1), (1, 4, 0, 1), (1, 1024, (1 << 19) + 1, 1),
                (1, 4, 4, 0), (1, 4, 4, 17)):
        assert lib.global_map_bytes(*bad) == 0
    assert lib.global_map_bytes(1, 1024, 1 << 19, 1) > 0
    with open(os.path.join(ROOT, "pwclonet_pylidarslam_amd", "csrc", "global_map.hpp")) as f:
        hpp = f.read()
    assert "GM_MAX_STREAMS = %d" % global_map.MAX_STREAMS in hpp and "GM_MAX_KEYFRAMES = %d" % global_map.MAX_KEYFRAMES in hpp
    assert "GM_MAX_ROWS = 1 << 29" in hpp and global_map.MAX_ROWS == 1 << 29 and "GM_BLOCK = %d" % global_map.BLOCK in hpp
    assert "GM_WORDS = %d" % global_map.WORDS in hpp


def test_kernels_reuse_the_grid_and_the_transform():
    with open(os.path.join(ROOT, "pwclonet_pylidarslam_amd", "csrc", "global_map.hip")) as f:
        src = f.read()
    for word in ('#include "grid.hpp"', '#include "se3.hpp"', "grid_key(", "grid_insert(", "grid_is_winner(", "se3_apply("):
        assert word in src, word
    assert "hipLaunchCooperativeKernel" not in src and "atomicAdd" not in src


# ---- host logic --------------------------------------------------------------------------------------------------------

def test_host_refusals():
    make = lambda **kw: global_map.GlobalMap(**dict(dict(streams=2, num_points=64), **kw))
    for kw in (dict(streams=0), dict(streams=1025), dict(num_points=0), dict(max_keyframes=0), dict(max_keyframes=65536),
               dict(max_keyframes=1024, num_points=(1 << 19) + 1), dict(voxel_size=0.0), dict(voxel_size=-1.0),
               dict(voxel_size=float("nan")), dict(voxel_size=float("inf")), dict(voxel_size="0.3"), dict(voxel_size=True),
               dict(capacity=0), dict(capacity=1024 * 64 + 1), dict(stride=0), dict(max_new=0), dict(max_new=1025)):
        with pytest.raises(ValueError, match="GlobalMap"):
            make(**kw)
    gm = make()
    assert gm.capacity == 1024 * 64 and make(num_points=8192).capacity == 1 << 22
    assert gm.map_bytes() == global_map.map_bytes(2, 1024, 64, 1024 * 64)
    assert gm.counts() is None and gm.totals() is None and gm.points(0) is None and not gm.overflowed() and gm.captures == 0
    gm.reset()
    cloud, poses = torch.zeros(2, 64, 3), torch.eye(4, dtype=torch.float64).expand(5, 2, 4, 4).contiguous()
    with pytest.raises(RuntimeError, match="CPU not supported"):
        gm.advance(cloud, [0, 0], poses)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        gm.rebuild(poses)
    for args in ((cloud.double(), [0, 0], poses), (torch.zeros(2, 63, 3), [0, 0], poses), (cloud, [0], poses),
                 (cloud, [0, -1], poses), (cloud, [0.0, 1.0], poses), (cloud, torch.zeros(2, dtype=torch.int64), poses),
                 (cloud, [0, 0], poses.float()), (cloud, [0, 0], poses[:, :1]), (cloud, [0, 0], poses[0]),
                 (cloud, [0, 0], poses[:0])):
        with pytest.raises(ValueError, match="GlobalMap"):
            gm.advance(*args)
    with pytest.raises(ValueError, match="lengths"):
        gm.advance(cloud, [0, 0], poses, lengths=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="active"):
        gm.advance(cloud, [0, 0], poses, active=[1])
    with pytest.raises(ValueError, match="rebuild"):
        gm.rebuild(poses[:, :1])
    for s in (-1, 2):
        with pytest.raises(ValueError, match="stream=%d" % s):
            gm.points(s)
        with pytest.raises(ValueError, match="stream=%d" % s):
            gm.reset([s])
    assert gm.bufs is None                                                   # nothing was allocated on the way
    clouds, X = torch.zeros(3, 8, 3), torch.eye(4, dtype=torch.float64).expand(3, 4, 4).contiguous()
    with pytest.raises(RuntimeError, match="CPU not supported"):
        global_map.build(clouds, X, 0.3)
    for args, kw in (((clouds, X, 0.0), {}), ((clouds, X, float("nan")), {}), ((clouds.double(), X, 0.3), {}),
                     ((clouds, X[:2], 0.3), {}), ((clouds, X.float(), 0.3), {}), ((clouds[:0], X[:0], 0.3), {}),
                     ((clouds, X, 0.3), dict(capacity=0)), ((clouds, X, 0.3), dict(capacity=25)),
                     ((clouds, X, 0.3), dict(lengths=torch.zeros(2, dtype=torch.int32))),
                     ((clouds, X, 0.3), dict(lengths=torch.zeros(3, dtype=torch.int64)))):
        with pytest.raises(ValueError, match="global_map.build"):
            global_map.build(*args, **kw)


def test_streaming_odometry_construction():
    so = StreamingOdometry(None, streams=2)
    assert so._map_cfg is None and so.global_map() is None
    with pytest.raises(RuntimeError, match="map="):
        so.map_points(0)
    with pytest.raises(ValueError, match="source=\"optimized\".*needs backend="):
        StreamingOdometry(None, streams=2, map=dict(source="optimized"))
    with pytest.raises(ValueError, match="source=\"refined\".*needs refine="):
        StreamingOdometry(None, streams=2, map=dict(source="refined"))
    with pytest.raises(ValueError, match="source="):
        StreamingOdometry(None, streams=2, map=dict(source="truth"))
    for key in ("streams", "num_points", "graph", "device"):
        with pytest.raises(ValueError, match="map=dict\\(%s" % key):
            StreamingOdometry(None, streams=2, map={key: 1})
    with pytest.raises(ValueError, match="map=dict\\(voxel="):
        StreamingOdometry(None, streams=2, map=dict(voxel=0.3))
    with pytest.raises(ValueError, match="rebuild_on_optimize"):
        StreamingOdometry(None, streams=2, backend=dict(), map=dict(rebuild_on_optimize=1))
    so = StreamingOdometry(None, streams=2, map=dict(voxel_size=0.5, stride=2))
    assert so._map_source == "network" and so._map_cfg == dict(voxel_size=0.5, stride=2) and so._map_rebuild is True
    assert so.global_map() is None and so.map_points(0) is None
    so = StreamingOdometry(None, streams=2, refine=dict(map_size=2), map=dict())
    assert so._map_source == "refined"
    so = StreamingOdometry(None, streams=2, refine=dict(map_size=2), backend=dict(), map=dict(rebuild_on_optimize=False))
    assert so._map_source == "optimized" and so._map_rebuild is False
    so = StreamingOdometry(None, streams=2, backend=dict(), map=dict(source="network"))
    assert so._map_source == "network"
