"""CPU tests of the motion compensation of raw sweeps: the NumPy model against the reference's rule
restated with SciPy, the model's own properties, every host-side refusal around ``times=``, and the new symbols'
declarations."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import deskew_model as model
from pwclonet_pylidarslam_amd import _lib, preprocess
from pwclonet_pylidarslam_amd.odometry import PWCLONetOdometry, StreamingOdometry
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cloud(n, seed):
    r = np.random.default_rng([seed, n])
    pts = (r.random((n, 3)) * [160.0, 160.0, 8.0] - [80.0, 80.0, 4.0]).astype(np.float32)
    times = 1.6e9 + np.sort(r.random(n)) * 0.1                      # a sweep of 0.1 s at an epoch time, fp64
    return pts, times


# ---- the model against SciPy ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(model.MOTIONS))
def test_model_is_the_references_slerp(name):
    rot = pytest.importorskip("scipy.spatial.transform")
    row = model.MOTIONS[name]
    pts, times = _cloud(2000, 3)
    # slam/preprocessing.py:177-190 on R = quat2mat(q), t: Slerp between the identity and R at the normalised times
    R = model.quat2mat(row[3:])
    slerp = rot.Slerp(np.array([0.0, 1.0]), rot.Rotation.from_matrix(np.array([np.eye(3), R])))
    alpha = (times - times.min()) / (times.max() - times.min())
    p = pts.astype(np.float64)
    t = row[:3].astype(np.float64)
    want = np.einsum("nij,nj->ni", slerp(alpha).as_matrix(), p) + alpha[:, None] * t[None]
    m, out = model.deskew(pts, times, row)
    tol = 1e-12 * (np.linalg.norm(p, axis=1) + np.linalg.norm(t))[:, None]
    assert (np.abs(m - want) <= tol).all(), float((np.abs(m - want) / tol).max())
    assert np.array_equal(out, m.astype(np.float32))
    if name not in ("0deg", "1e-9deg", "nq<1e-8"):
        assert np.abs(want - p - alpha[:, None] * t[None]).max() > 0.1          # the rotation is really there


# ---- the model's properties --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(model.MOTIONS))
def test_the_last_row_gets_the_whole_motion(name):
    row = model.MOTIONS[name]
    pts, times = _cloud(500, 5)
    m, _ = model.deskew(pts, times, row)
    last = int(np.argmax(times))
    p = pts[last].astype(np.float64)
    want = model.quat2mat(row[3:]) @ p + row[:3].astype(np.float64)
    assert np.abs(m[last] - want).max() <= 1e-12 * (np.linalg.norm(p) + np.linalg.norm(row[:3]))
    first = int(np.argmin(times))
    assert np.array_equal(m[first], pts[first].astype(np.float64))            # alpha = 0


def test_identity_motion_and_equal_times_return_the_input_bits():
    pts, times = _cloud(300, 7)
    pts[5] = [-0.0, 0.0, -0.0]                                                # signed zeros keep their sign
    pts[6] = [np.nan, np.inf, -np.inf]
    for row in (model.IDENTITY, np.array([0, 0, 0, -3, 0, 0, 0], np.float32), np.array([0, 0, 0, 1e-6, 0, 0, 0], np.float32)):
        _, out = model.deskew(pts, times, row)
        assert np.array_equal(out.view(np.uint32), pts.view(np.uint32))
    for row in model.MOTIONS.values():
        _, out = model.deskew(pts, np.full(300, 7.25), row)                   # tau_max == tau_min
        assert np.array_equal(out.view(np.uint32), pts.view(np.uint32))
        alpha, _ = model.alphas(np.full(300, np.nan))                         # no finite time at all
        assert not alpha.any()
    assert not model.alphas(np.array([3.0]))[0].any()                         # one row


def test_a_kept_row_without_a_finite_time_stays_where_it_is():
    pts, times = _cloud(400, 9)
    times[[10, 200, 399]] = [np.nan, np.inf, -np.inf]
    alpha, cand = model.alphas(times)
    assert cand.all() and not alpha[[10, 200, 399]].any()
    clean = np.delete(times, [10, 200, 399])
    assert np.array_equal(np.delete(alpha, [10, 200, 399]), model.alphas(clean)[0])     # and moves nobody else
    _, out = model.deskew(pts, times, model.MOTIONS["90deg"])
    assert np.array_equal(out[[10, 200, 399]], pts[[10, 200, 399]])
    assert alpha.min() == 0.0 and alpha.max() == 1.0


def test_times_of_dropped_rows_and_rows_past_the_length_do_not_count():
    pts, times = _cloud(600, 11)
    keep = (np.arange(600) % 3 != 0).astype(np.int32)
    want_alpha, _ = model.alphas(times[:500][keep[:500] != 0])
    planted = times.copy()
    planted[keep == 0] = np.resize([-1e300, 1e300, np.nan], 200)               # on the rows the filter drops
    planted[500:] = [1e300, -1e300] * 50                                       # and past the length
    alpha, cand = model.alphas(planted, keep=keep, length=500)
    assert np.array_equal(alpha[:500][keep[:500] != 0], want_alpha)
    assert not alpha[~cand].any() and cand.sum() == (keep[:500] != 0).sum()
    _, out = model.deskew(pts, planted, model.MOTIONS["2deg"], keep=keep, length=500)
    assert np.array_equal(out[~cand], pts[~cand])                              # non-candidates pass through
    assert (out[cand] != pts[cand]).any()


def test_bound_is_half_an_ulp_plus_fp64_noise():
    assert model.ulp32(1.0) == 2.0 ** -23 and model.ulp32(0.99) == 2.0 ** -24 and model.ulp32(0.0) == 2.0 ** -149
    assert model.ulp32(-80.0) == np.spacing(np.float32(80.0))
    m = np.array([[1.5, -80.0, 0.0]])
    b = model.bound(m, np.float32([[3, 4, 0]]), model.IDENTITY)
    assert np.allclose(b, 0.5 * model.ulp32(m) + 5e-12, rtol=1e-15, atol=0)


# ---- host checks, no GPU -------------------------------------------------------------------------------------------------------

def _cpu_net():
    return PWCLONet(dict(num_input_channels=3, sequence_len=2, device="cpu", scalar_last=False, log_mode="none")).eval()


@pytest.mark.parametrize("per_stream", [False, True])
def test_times_belong_to_deskew_and_to_nothing_else(per_stream):
    sweeps = torch.zeros(2, 100, 4)
    times = torch.zeros(2, 100, dtype=torch.float64)
    on = StreamingOdometry(_cpu_net(), streams=2, graph=False, per_stream=per_stream,
                           sweeps=dict(dataset="kitti360", capacity=4096, deskew=True))
    off = StreamingOdometry(_cpu_net(), streams=2, graph=False, per_stream=per_stream,
                            sweeps=dict(dataset="kitti360", capacity=4096))
    assert on.motion() is None and off.motion() is None                       # nothing allocated yet
    with torch.no_grad():
        with pytest.raises(ValueError, match="deskew=True"):
            off.step_sweeps(sweeps, [100, 100], times=times)
        with pytest.raises(ValueError, match="times="):
            on.step_sweeps(sweeps, [100, 100])
        for bad in (times[:, :99], times[:1], times.reshape(-1), times[:, :, None]):
            with pytest.raises(ValueError, match="times must be"):
                on.step_sweeps(sweeps, [100, 100], times=bad)
        for bad in (times.long(), times.to(torch.int32), times.bool(), times.numpy()):
            with pytest.raises(ValueError, match="floating"):
                on.step_sweeps(sweeps, [100, 100], times=bad)
        with pytest.raises(RuntimeError, match="CPU not supported"):              # well formed, but on the host
            on.step_sweeps(sweeps, [100, 100], times=times.float())
    assert on._front.bufs is None and on.frames_seen == 0


def test_front_end_and_eager_chain_refusals():
    with pytest.raises(ValueError, match="deskew"):
        preprocess.SweepFrontEnd(1, 256, capacity=4096, deskew="yes")
    front = preprocess.SweepFrontEnd(2, 256, capacity=4096, deskew=True)
    with pytest.raises(ValueError, match="times="):
        front.check_times(None, torch.zeros(2, 10, 4), "test")
    with pytest.raises(ValueError, match="both"):
        preprocess.frames_to_clouds(torch.zeros(1, 100, 4), 16, "kitti360", times=torch.zeros(1, 100))
    with pytest.raises(ValueError, match="both"):
        preprocess.frames_to_clouds(torch.zeros(1, 100, 4), 16, "kitti360", motion=torch.zeros(1, 7))
    pts, ident = torch.zeros(2, 50, 3), torch.tensor(model.IDENTITY).repeat(2, 1)
    with pytest.raises(ValueError, match="times must be"):
        preprocess.deskew(pts, torch.zeros(2, 49), ident)
    with pytest.raises(ValueError, match="floating"):
        preprocess.deskew(pts, torch.zeros(2, 50, dtype=torch.int64), ident)
    with pytest.raises(ValueError, match="motion"):
        preprocess.deskew(pts, torch.zeros(2, 50), ident[:1])
    with pytest.raises(ValueError, match="motion"):
        preprocess.deskew(pts, torch.zeros(2, 50), ident.double())
    with pytest.raises(ValueError, match="points"):
        preprocess.deskew(torch.zeros(2, 50, 5), torch.zeros(2, 50), ident)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        preprocess.deskew(pts, torch.zeros(2, 50), ident)


def test_the_front_end_buffers_with_deskew():
    front = preprocess.SweepFrontEnd(2, 256, capacity=4096, deskew=True)
    plain = preprocess.SweepFrontEnd(2, 256, capacity=4096)
    front._alloc(torch.device("cpu"))
    plain._alloc(torch.device("cpu"))
    assert set(front.bufs) - set(plain.bufs) == {"times", "motion"}
    assert front.bufs["times"].shape == (2, 4096) and front.bufs["times"].dtype == torch.float64
    assert front.bufs["times"].numel() * 8 // 2 == 4096 * 8                     # 8 bytes per row and stream
    assert torch.equal(front.bufs["motion"], torch.tensor(model.IDENTITY).repeat(2, 1))
    front.load(torch.zeros(2, 10, 4), None, [10, 10], torch.arange(20, dtype=torch.float32).reshape(2, 10))
    assert front.bufs["times"][1, :10].tolist() == list(range(10, 20)) and not front.bufs["times"][:, 10:].any()


def test_odometry_wrapper_reads_the_references_timestamps_key():
    od = PWCLONetOdometry(dict(num_input_channels=3, sequence_len=2, num_points=64), device="cpu",
                          sweeps=dict(dataset="kitti360", capacity=2048, deskew=True))
    assert od.timestamps_key() == "numpy_pc_timestamps" and od.stream._front.deskew
    frame = torch.zeros(1, 30, 4)
    ts = od._times({"numpy_pc_timestamps": np.linspace(0.0, 0.1, 30)}, frame)
    assert ts.shape == (1, 30) and ts.dtype == torch.float64
    none = od._times({}, frame)                                                # no key: equal times, nobody moves
    assert none.shape == (1, 30) and not none.any()
    with pytest.raises(ValueError, match="one floating time per row"):
        od._times({"numpy_pc_timestamps": np.zeros(29)}, frame)
    plain = PWCLONetOdometry(dict(num_input_channels=3, sequence_len=2, num_points=64), device="cpu",
                             sweeps=dict(dataset="kitti360", capacity=2048))
    assert plain._times({"numpy_pc_timestamps": np.zeros(30)}, frame) is None


# ---- declarations ----------------------------------------------------------------------------------------------------------

NEW = [("deskew_rows_kernel_wrapper", 9), ("sweep_filter_deskew_compact_kernel_wrapper", 15),
       ("sweep_filter_deskew_grid_compact_kernel_wrapper", 18), ("stream_motion_handover_kernel_wrapper", 5)]


@pytest.mark.parametrize("name, arity", NEW)
def test_new_symbols_are_declared_with_the_header_arity(name, arity):
    args, res = _lib.SIGNATURES[name]
    with open(os.path.join(ROOT, "include", "pwclo_ops.h")) as f:
        header = f.read()
    m = re.search(r"void\s+%s\s*\(([^)]*)\)\s*;" % name, header)
    assert m is not None, "%s is not declared in include/pwclo_ops.h" % name
    assert res is None
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(args) == len(params) == arity
    for p, a in zip(params, args):
        want = _lib._F if "*" in p else ctypes.c_float if p.startswith("float") else \
            ctypes.c_double if p.startswith("double") else _lib._i
        assert a is want, (p, a)
    assert hasattr(_lib.load(), name)
    assert _lib.load().pwclo_abi_version() == 1                                 # additions only: the version stays


def test_fused_wrappers_extend_the_old_ones_and_leave_them_alone():
    sig = lambda n: _lib.SIGNATURES[n][0]
    old, grid = sig("sweep_filter_compact_kernel_wrapper"), sig("sweep_filter_grid_compact_kernel_wrapper")
    new, newgrid = sig("sweep_filter_deskew_compact_kernel_wrapper"), sig("sweep_filter_deskew_grid_compact_kernel_wrapper")
    assert len(old) == 11 and len(grid) == 14
    assert new[:9] == old[:9] and new[9:13] == [_lib._F] * 4 and new[13:] == old[9:]       # times, motion, restart, have_prev
    assert newgrid[:9] == grid[:9] and newgrid[9:13] == [_lib._F] * 4 and newgrid[13:] == grid[9:]
