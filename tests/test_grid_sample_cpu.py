"""CPU tests of voxel grid sampling: the NumPy model against the rule restated by hand, the new
symbols' declarations, every host-side refusal, and the buffers the raw front end allocates with and without a grid."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import grid_sample_model as model
from pwclonet_pylidarslam_amd import _lib, preprocess
from pwclonet_pylidarslam_amd.odometry import PWCLONetOdometry, StreamingOdometry
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cloud(values):
    return np.asarray(values, dtype=np.float32)


# ---- the model ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed, n, v", [(0, 1, 0.3), (1, 500, 0.3), (2, 4000, 0.5), (3, 4000, 2.0)])
def test_model_winners_are_the_first_row_of_every_hash(seed, n, v):
    rng = np.random.default_rng(seed)
    pts = (rng.random((n, 3)) * [20.0, 20.0, 4.0] - [10.0, 10.0, 2.0]).astype(np.float32)
    h, ok = model.voxel_hash(pts, v)
    assert ok.all()
    got = np.flatnonzero(model.grid_keep(pts, v))
    assert np.array_equal(got, np.sort(np.unique(h, return_index=True)[1]))
    # the same without np.unique, on the voxel coordinates themselves: no two voxels of such a cloud share a hash
    seen, first = set(), []
    q = np.rint(pts.astype(np.float64) / v).astype(np.int64)
    for i, key in enumerate(map(tuple, q)):
        if key not in seen:
            seen.add(key)
            first.append(i)
    assert got.tolist() == first
    if n >= 4000:
        assert 1 < len(first) < n                          # some rows share a voxel, some do not


def test_half_way_points_round_to_even():
    # v = 0.5: 0.25 / 0.5 = 0.5 -> 0, 0.75 / 0.5 = 1.5 -> 2, -0.25 / 0.5 = -0.5 -> -0, 1.25 / 0.5 = 2.5 -> 2,
    # -0.75 / 0.5 = -1.5 -> -2, -1.25 / 0.5 = -2.5 -> -2 (all exact in fp32 and fp64)
    xs = _cloud([0.25, 0.75, -0.25, 1.25, -0.75, -1.25])
    pts = np.zeros((6, 3), dtype=np.float32)
    pts[:, 0] = xs
    h, ok = model.voxel_hash(pts, 0.5)
    assert ok.all()
    assert h.tolist() == [73856093 * q for q in (0, 2, 0, 2, -2, -2)]
    assert model.grid_keep(pts, 0.5).tolist() == [1, 1, 0, 0, 1, 0]
    # the other axes carry their own primes
    pts = _cloud([[0.0, 0.75, 0.0], [0.0, 0.0, 1.25], [0.0, 1.25, 0.0]])
    assert model.voxel_hash(pts, 0.5)[0].tolist() == [19349669 * 2, 83492791 * 2, 19349669 * 2]
    assert model.grid_keep(pts, 0.5).tolist() == [1, 1, 0]


def test_signed_zeros_share_a_voxel():
    pts = _cloud([[-0.0, 0.0, -0.0], [0.0, -0.0, 0.0], [0.1, -0.1, 0.1], [-0.14, 0.0, 0.0]])
    h, ok = model.voxel_hash(pts, 0.3)
    assert ok.all() and h.tolist() == [0, 0, 0, 0]
    assert model.grid_keep(pts, 0.3).tolist() == [1, 0, 0, 0]


def test_non_finite_and_out_of_range_rows_are_dropped():
    big = np.float32(2.0 ** 31)                           # |p / v| = 2^31 at v = 1: out; the float below it: in
    below = np.nextafter(big, np.float32(0))
    pts = _cloud([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [big, 0, 0], [0, -big, 0], [below, 0, 0], [1, 1, 1],
                  [np.nan, 0, 0], [1, 1, 1]])
    h, ok = model.voxel_hash(pts, 1.0)
    assert ok.tolist() == [False, False, False, False, False, True, True, False, True]
    assert model.grid_keep(pts, 1.0).tolist() == [0, 0, 0, 0, 0, 1, 1, 0, 0]
    assert h[5] == 73856093 * int(below)
    # a smaller voxel moves the limit: 2^30 / 0.25 = 2^32
    assert model.grid_keep(_cloud([[2.0 ** 30, 0, 0], [3.0, 0, 0]]), 0.25).tolist() == [0, 1]
    # length and keep: rows outside are no candidates, so a later row of the voxel wins
    pts = _cloud([[1, 1, 1], [1, 1, 1], [5, 5, 5], [1, 1, 1]])
    assert model.grid_keep(pts, 0.5, keep=[0, 1, 1, 1]).tolist() == [0, 1, 1, 0]
    assert model.grid_keep(pts, 0.5, length=1).tolist() == [1, 0, 0, 0]
    assert model.grid_keep(pts, 0.5, length=0).tolist() == [0, 0, 0, 0]


def test_the_empty_slot_marker_is_a_reachable_hash():
    q = model.solve_hash(model.EMPTY_KEY)
    assert q is not None and max(map(abs, q)) <= 1 << 24
    assert sum(p * x for p, x in zip(model.PRIMES, q)) == -1
    pts = _cloud([q, q, [0, 0, 0]])                     # v = 1: the coordinates are the voxel indices, exact in fp32
    h, ok = model.voxel_hash(pts, 1.0)
    assert ok.all() and h.tolist() == [-1, -1, 0]
    assert model.grid_keep(pts, 1.0).tolist() == [1, 0, 1]


# ---- declarations --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, arity", [("grid_sample_workspace_bytes", 2), ("grid_sample_keep_kernel_wrapper", 10),
                                         ("sweep_filter_grid_compact_kernel_wrapper", 14)])
def test_new_symbols_are_declared_with_the_header_arity(name, arity):
    args, res = _lib.SIGNATURES[name]
    with open(os.path.join(ROOT, "include", "pwclo_ops.h")) as f:
        header = f.read()
    m = re.search(r"(void|long long)\s+%s\s*\(([^)]*)\)\s*;" % name, header)
    assert m is not None, "%s is not declared in include/pwclo_ops.h" % name
    assert res is (None if m.group(1) == "void" else ctypes.c_longlong)
    params = [p.strip() for p in m.group(2).split(",")]
    assert len(args) == len(params) == arity
    for p, a in zip(params, args):
        want = _lib._F if "*" in p else ctypes.c_float if p.startswith("float") else \
            ctypes.c_double if p.startswith("double") else _lib._i
        assert a is want, (p, a)


def test_fused_wrapper_extends_the_old_one_and_leaves_it_alone():
    old = _lib.SIGNATURES["sweep_filter_compact_kernel_wrapper"][0]
    new = _lib.SIGNATURES["sweep_filter_grid_compact_kernel_wrapper"][0]
    assert len(old) == 11
    assert new[:9] == old[:9] and new[9] is ctypes.c_double and new[10] is _lib._F      # ..., voxel, workspace,
    assert new[11:13] == old[9:11] and new[13] is _lib._F                               # packed, counts, winners


def test_workspace_bytes():
    lib = _lib.load()
    one = lib.grid_sample_workspace_bytes(1, 131072)
    # 2^18 slots of a 64-bit key and a 32-bit row word (+ 2 words), and a 32-bit word per row
    assert one == (1 << 18) * 12 + 8 + 131072 * 4
    assert lib.grid_sample_workspace_bytes(8, 131072) == 8 * one and one % 8 == 0
    assert lib.grid_sample_workspace_bytes(1, 1) == 64 * 12 + 8 + 16                    # never fewer than 64 slots
    assert lib.grid_sample_workspace_bytes(3, 5000) % 8 == 0
    for b, n in ((0, 10), (1, 0), (1, (1 << 20) + 1)):
        assert lib.grid_sample_workspace_bytes(b, n) == 0


# ---- refusals ------------------------------------------------------------------------------------------------------------

BAD_VOXELS = [0, 0.0, -0.3, float("nan"), float("inf"), "0.3", True]


def _cpu_net():
    return PWCLONet(dict(num_input_channels=3, sequence_len=2, device="cpu", scalar_last=False, log_mode="none")).eval()


@pytest.mark.parametrize("bad", BAD_VOXELS, ids=repr)
def test_voxel_size_must_be_a_finite_positive_number(bad):
    with pytest.raises(ValueError, match="voxel_size"):
        preprocess.SweepFrontEnd(1, 256, capacity=4096, voxel_size=bad)
    with pytest.raises(ValueError, match="voxel_size"):
        StreamingOdometry(_cpu_net(), streams=1, graph=False, sweeps=dict(dataset="kitti360", capacity=4096, voxel_size=bad))
    with pytest.raises(ValueError, match="voxel_size"):
        preprocess.frames_to_clouds(torch.zeros(1, 100, 4), 16, "kitti360", voxel_size=bad)    # before the device check
    with pytest.raises(ValueError, match="voxel_size"):
        preprocess.grid_sample(torch.zeros(100, 3), bad)


def test_voxel_capacity_range_and_dependence():
    for bad in (0, -1, 4097, 2.5, True):
        with pytest.raises(ValueError, match="voxel_capacity"):
            preprocess.SweepFrontEnd(1, 256, capacity=4096, voxel_size=0.3, voxel_capacity=bad)
    with pytest.raises(ValueError, match="voxel_capacity"):
        preprocess.SweepFrontEnd(1, 256, capacity=4096, voxel_capacity=1024)              # no voxel_size
    with pytest.raises(ValueError, match="voxel_capacity"):
        preprocess.frames_to_clouds(torch.zeros(1, 100, 4), 16, "kitti360", voxel_capacity=50)
    with pytest.raises(ValueError, match="voxel_capacity"):
        preprocess.frames_to_clouds(torch.zeros(1, 100, 4), 16, "kitti360", voxel_size=0.3, voxel_capacity=101)
    with pytest.raises(ValueError, match="voxel_capacity"):
        preprocess.frames_to_clouds(torch.zeros(1, 100, 4), 16, "kitti360", cap=60, voxel_size=0.3, voxel_capacity=61)
    with pytest.raises(ValueError, match="voxel_capacity"):
        StreamingOdometry(_cpu_net(), streams=2, graph=False, per_stream=True,
                          sweeps=dict(dataset="kitti360", capacity=4096, voxel_size=0.3, voxel_capacity=0))
    with pytest.raises(ValueError, match="voxel_capacity"):
        PWCLONetOdometry(dict(num_input_channels=3, sequence_len=2, num_points=64), device="cpu",
                         sweeps=dict(dataset="kitti360", capacity=2048, voxel_capacity=100))
    for ok in (1, 4096):
        front = preprocess.SweepFrontEnd(1, 256, capacity=4096, voxel_size=0.3, voxel_capacity=ok)
        assert front.width == ok and front.capacity == 4096 and front.voxel_size == 0.3
    assert preprocess.SweepFrontEnd(1, 256, capacity=4096, voxel_size=np.float32(0.5)).width == 4096


def test_the_stream_limit_follows_the_packed_width():
    # 131072-row sweeps: 24 streams per launch of the large-cloud sampler; grid-sampled to <= 24576 rows there is no limit
    with pytest.raises(ValueError, match="co-resident"):
        preprocess.SweepFrontEnd(25, 8192, capacity=131072)
    with pytest.raises(ValueError, match="co-resident"):
        preprocess.SweepFrontEnd(25, 8192, capacity=131072, voxel_size=0.3)               # voxel_capacity = capacity
    preprocess.SweepFrontEnd(25, 8192, capacity=131072, voxel_size=0.3, voxel_capacity=24576)
    so = StreamingOdometry(_cpu_net(), streams=32, graph=False,
                           sweeps=dict(dataset="kitti360", capacity=131072, voxel_size=0.3, voxel_capacity=24576))
    assert so.voxel_counts() is None and so.survivor_counts() is None                     # nothing allocated yet


def test_grid_sample_argument_checks():
    with pytest.raises(RuntimeError, match="CPU not supported"):
        preprocess.grid_sample(torch.zeros(100, 3), 0.3)
    with pytest.raises(ValueError, match="voxel_size"):
        preprocess.grid_sample(torch.zeros(100, 3), None)


# ---- buffers -----------------------------------------------------------------------------------------------------------

def _shapes(front):
    front._alloc(torch.device("cpu"))
    return {k: (tuple(v.shape), v.dtype) for k, v in front.bufs.items() if v is not None}


def _todays(S, cap, m, kitti):
    """What SweepFrontEnd._alloc makes without a grid, written down from the parent's code."""
    want = dict(sweeps=((S, cap, 4), torch.float32), lengths=((S,), torch.int32), packed=((S, cap, 3), torch.float32),
                counts=((S,), torch.int32), idx=((S, m), torch.int32))
    if kitti:
        want["tr"] = ((S, 3, 4), torch.float64)
    if cap > 24576:
        want["tmp"] = ((S, cap), torch.float32)
    if cap >= 32768:
        want["order_ws"] = ((_lib.load().fps_spatial_order_workspace_bytes(S, cap),), torch.uint8)
        want["sorted"] = ((S, cap, 3), torch.float32)
        want["perm"] = ((S, cap), torch.int32)
    return want


@pytest.mark.parametrize("cap", [4096, 24576, 24577, 32767, 32768, 40000])
@pytest.mark.parametrize("dataset", ["kitti360", "kitti"])
def test_without_a_grid_the_front_end_allocates_todays_buffers(cap, dataset):
    tr = np.eye(4)[:3] if dataset == "kitti" else None
    front = preprocess.SweepFrontEnd(2, 256, dataset=dataset, capacity=cap, tr=tr)
    assert front.voxel_size is None and front.width == cap
    assert _shapes(front) == _todays(2, cap, 256, dataset == "kitti")
    assert front.voxel_counts() is None


@pytest.mark.parametrize("cap, width", [(4096, 4096), (40000, 4096), (40000, 24576), (40000, 30000), (40000, 40000)])
def test_with_a_grid_the_sampler_buffers_follow_the_packed_width(cap, width):
    front = preprocess.SweepFrontEnd(2, 256, capacity=cap, voxel_size=0.3, voxel_capacity=width)
    got = _shapes(front)
    want = _todays(2, width, 256, False)
    want["sweeps"] = ((2, cap, 4), torch.float32)                  # the raw rows keep the sweep capacity
    want["grid_ws"] = ((_lib.load().grid_sample_workspace_bytes(2, cap) // 8,), torch.int64)
    want["winners"] = ((2,), torch.int32)
    assert got == want
    assert ("tmp" in got) == (width > 24576) and ("order_ws" in got) == (width >= 32768)
    assert front.voxel_counts() is front.bufs["winners"]
