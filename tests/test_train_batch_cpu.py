"""CPU tests of the device-side training batch builder (``batches.TrainBatchBuilder``): the Philox
generator of the host model against the Random123 known answers, the LAW of the model's draws at fixed seeds (so the tests
are deterministic), its pose algebra against independent code (``oracle/eval_oracle.py``, scipy), the builder's host-side
refusals, and the ABI of the two new launchers.  The GPU tests compare the kernels with this model bit for bit."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_batch_model as model                                             # noqa: E402

from pwclonet_pylidarslam_amd import _lib                                     # noqa: E402
from pwclonet_pylidarslam_amd.batches import TrainBatchBuilder, pad_pairs     # noqa: E402

VELO_TO_CAM = [[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0], [1.0, 0.0, 0.0, 0.0]]


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    cases = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
             ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
             ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
              "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in cases:
        got = " ".join("%08x" % int(v) for v in model.philox4x32_10(ctr, key))
        assert got == want, (ctr, key, got)
    # vectorised over the index like the selection uses it: same words as one call per index
    w = model.words(np.arange(5), 3, 7, model.SELECT, seed=(9 << 32) | 5)
    for i in range(5):
        assert int(w[i]) == int(model.philox4x32_10((i, 3, 7, 0), (5, 9))[0])


def test_selection_is_a_uniform_subset_in_random_order():
    from scipy.stats import chi2
    n, npoints, steps, bins = 96000, 8192, 200, 96
    keep = np.ones(n, dtype=bool)
    keep[::7] = False                                                          # survivors are not all rows
    hist = np.zeros(bins)
    first = []
    for step in range(steps):
        rows, count = model.select_rows(keep, npoints, cloud=5, step=step, seed=1234)
        assert count == int(keep.sum()) and rows.shape == (npoints,)
        assert len(np.unique(rows)) == npoints and keep[rows].all()
        hist += np.bincount(rows // (n // bins), minlength=bins)
        first.append(rows[0])
    per_bin = np.bincount(np.nonzero(keep)[0] // (n // bins), minlength=bins)
    expect = hist.sum() * per_bin / per_bin.sum()
    stat = float(((hist - expect) ** 2 / expect).sum())
    print("chi-square of the selection counts over %d bins: %.1f (0.999 quantile %.1f)" % (bins, stat, chi2.ppf(0.999, bins - 1)))
    assert stat < chi2.ppf(0.999, bins - 1)
    # random ORDER: the first output point's row is spread over the scan (uniform on [0, n): mean n/2, sd n/sqrt(12))
    first = np.array(first)
    assert abs(first.mean() - n / 2) < 4 * n / np.sqrt(12 * steps)
    assert first.min() < n / 10 and first.max() > n * 9 / 10
    # a different step, cloud or seed gives a different subset
    base = model.select_rows(keep, npoints, 5, 0, 1234)[0]
    for kw in (dict(cloud=5, step=1, seed=1234), dict(cloud=6, step=0, seed=1234), dict(cloud=5, step=0, seed=1235)):
        assert not np.array_equal(base, model.select_rows(keep, npoints, **kw)[0])


def test_selection_with_too_few_survivors():
    n, npoints = 5000, 1024
    keep = np.zeros(n, dtype=bool)
    keep[100:400] = True
    rows, count = model.select_rows(keep, npoints, 0, 3, 7)
    assert count == 300 and np.array_equal(rows[:300], np.arange(100, 400))
    assert keep[rows].all() and len(np.unique(rows[300:])) > 200               # draws with replacement over the survivors
    rows, count = model.select_rows(np.zeros(n, dtype=bool), npoints, 0, 3, 7)
    assert count == 0 and rows.min() >= 0 and rows.max() < n and rows.max() > n * 0.9


def test_augmentation_law():
    """Each parameter is fp32(clip(scale * z)), z standard normal: inside the clips, clipped fraction 2 * Phi(-clip / scale),
    mean 0; both within 4 standard errors over 20 000 draws."""
    from scipy.stats import norm
    draws = np.stack([model.draw_aug(pair, step, seed=99) for step in range(100) for pair in range(200)])
    assert draws.shape == (20000, 6) and draws.dtype == np.float32
    N = draws.shape[0]
    for j in range(6):
        s, c = model.AUG_SCALE[j], model.AUG_CLIP[j]
        x = draws[:, j].astype(np.float64)
        assert np.all(np.abs(x) <= np.float32(c))
        a = c / s
        p_clip = 2 * norm.cdf(-a)
        var = s * s * ((1 - p_clip) - 2 * a * norm.pdf(a)) + c * c * p_clip    # clipped-normal variance (mean 0)
        frac = np.mean(np.abs(x) >= np.float32(c))
        print("param %d: mean %.3g (se %.3g), clipped %.4f (law %.4f)" % (j, x.mean(), np.sqrt(var / N), frac, p_clip))
        assert abs(x.mean()) < 4 * np.sqrt(var / N)
        assert abs(frac - p_clip) < 4 * np.sqrt(p_clip * (1 - p_clip) / N)
    assert np.array_equal(model.draw_aug(3, 5, 99), model.draw_aug(3, 5, 99))
    assert not np.array_equal(model.draw_aug(3, 5, 99), model.draw_aug(3, 6, 99))


def _random_t_diff(rng):
    from scipy.spatial.transform import Rotation
    T = np.eye(4)
    T[:3, :3] = Rotation.from_rotvec(rng.normal(0, 0.05, 3)).as_matrix()
    T[:3, 3] = rng.normal(0, 1.0, 3)
    return T


def test_pose_algebra_against_independent_code():
    from scipy.spatial.transform import Rotation
    from oracle import eval_oracle
    rng = np.random.default_rng(5)
    for trial in range(50):
        Td = _random_t_diff(rng)
        params = model.draw_aug(trial, 0, seed=11)
        Tt, Tg, gt = model.pose("kitti", Td, params)
        assert np.abs(Tt[:3, :3] @ Tt[:3, :3].T - np.eye(3)).max() < 1e-15 and np.array_equal(Tt[3], [0, 0, 0, 1])
        assert np.abs(Tg @ Tt - Td).max() < 1e-12                                      # T_gt . T_trans == T_diff
        q = model.quat_zyx(Tg[:3, :3])
        assert np.abs(eval_oracle.quat2mat(q) - Tg[:3, :3]).max() < 1e-12
        assert np.array_equal(gt, np.concatenate([Tg[:3, 3], q]).astype(np.float32))
        Tt, Tg, gt = model.pose("kitti360", Td, params)
        assert np.abs(Tg - Tt @ Td).max() < 1e-15
        q = model.quat_diag(Tg[:3, :3])
        assert np.abs(eval_oracle.quat2mat(q) - Tg[:3, :3]).max() < 1e-12
        sq = Rotation.from_matrix(Tg[:3, :3]).as_quat()
        assert np.abs(q - np.concatenate([sq[3:], sq[:3]])).max() <= 1e-15
        assert np.array_equal(gt, np.concatenate([Tg[:3, 3], q]).astype(np.float32))
        # no augmentation: T_gt is T_diff itself
        for ds in ("kitti", "kitti360"):
            Tt, Tg, _ = model.pose(ds, Td[:3], None)
            assert np.array_equal(Tt, np.eye(4)) and np.array_equal(Tg, Td)
    # the quaternion forms away from the small-angle case: every branch of the largest-diagonal form
    for rotvec in ([3.0, 0.1, 0.2], [0.1, 3.0, 0.2], [0.1, 0.2, 3.0], [0.3, -0.2, 0.1]):
        Rm = Rotation.from_rotvec(rotvec).as_matrix()
        sq = Rotation.from_matrix(Rm).as_quat()
        assert np.abs(model.quat_diag(Rm) - np.concatenate([sq[3:], sq[:3]])).max() <= 1e-15
        assert np.abs(eval_oracle.quat2mat(model.quat_zyx(Rm)) - Rm).max() < 1e-12


def test_model_batch_follows_the_dataset_conventions():
    """KITTI hands the pair over swapped (xyz_f1 = augmented pc2), KITTI-360 in order; both frames use the shorter length."""
    rng = np.random.default_rng(3)
    sweeps = rng.uniform(-20, 20, (2, 2, 600, 4)).astype(np.float32)
    sweeps[..., 2] = rng.uniform(-1.0, 1.0, (2, 2, 600))
    lengths = np.array([[600, 500], [450, 600]])
    Td = np.stack([_random_t_diff(rng) for _ in range(2)])
    for ds, tr in (("kitti", VELO_TO_CAM), ("kitti360", None)):
        out = model.build(ds, sweeps, lengths, Td, 256, seed=4, step=2, tr=tr)
        assert out["indices"].max() < 500 and out["indices"][2:].max() < 450
        for b in range(2):
            n = lengths[b].min()
            xyz0, _ = model.filter_rows(ds, sweeps[b, 0, :n], tr)
            xyz1, _ = model.filter_rows(ds, sweeps[b, 1, :n], tr)
            plain = xyz0[out["indices"][2 * b]].T
            moved = model.apply_trans(out["t_trans"][b], xyz1[out["indices"][2 * b + 1]]).T
            first, second = (moved, plain) if ds == "kitti" else (plain, moved)
            assert np.array_equal(out["xyz_f1"][b], first) and np.array_equal(out["xyz_f2"][b], second)


def test_builder_refuses_bad_arguments_on_the_host(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("a library call was made before the host checks finished")
    monkeypatch.setattr(_lib, "call", no_library)
    monkeypatch.setattr(_lib, "load", no_library)
    with pytest.raises(ValueError, match="tr"):
        TrainBatchBuilder(2, dataset="kitti")
    with pytest.raises(ValueError, match="dataset"):
        TrainBatchBuilder(2, dataset="nuscenes")
    with pytest.raises(ValueError, match="npoints"):
        TrainBatchBuilder(2, dataset="kitti360", npoints=16384)
    with pytest.raises(ValueError, match="capacity"):
        TrainBatchBuilder(2, dataset="kitti360", capacity=0)
    with pytest.raises(ValueError, match="tr must be"):
        TrainBatchBuilder(2, dataset="kitti", tr=np.zeros((3, 3, 4)))
    bld = TrainBatchBuilder(2, dataset="kitti360", npoints=64, capacity=512)
    sweeps = torch.zeros(2, 2, 256, 4)
    lengths = [[256, 200], [100, 256]]
    td = torch.eye(4, dtype=torch.float64).repeat(2, 1, 1)
    with pytest.raises(ValueError, match="float32"):
        bld.build(sweeps.double(), lengths, td)
    with pytest.raises(ValueError, match="2 frames of 4 channels"):
        bld.build(torch.zeros(2, 2, 256, 3), lengths, td)
    with pytest.raises(ValueError, match="built for 2 pairs"):
        bld.build(torch.zeros(3, 2, 256, 4), lengths, td)
    with pytest.raises(ValueError, match="capacity=512"):
        bld.build(torch.zeros(2, 2, 600, 4), lengths, td)
    with pytest.raises(ValueError, match=r"outside \[1, 256\]"):
        bld.build(sweeps, [[256, 0], [100, 256]], td)
    with pytest.raises(ValueError, match=r"outside \[1, 256\]"):
        bld.build(sweeps, [[257, 1], [100, 256]], td)
    with pytest.raises(ValueError, match="lengths must be"):
        bld.build(sweeps, [256, 200], td)
    with pytest.raises(ValueError, match="lengths must be"):
        bld.build(sweeps, [[256.0, 200.0], [1.0, 2.0]], td)
    with pytest.raises(ValueError, match="t_diff must be float64"):
        bld.build(sweeps, lengths, td.float())
    with pytest.raises(ValueError, match="t_diff must be float64"):
        bld.build(sweeps, lengths, td[:1])
    with pytest.raises(ValueError, match="aug must be"):
        bld.build(sweeps, lengths, td, aug=torch.zeros(2, 5))
    with pytest.raises(ValueError, match="out xyz_f1"):
        bld.build(sweeps, lengths, td, out=(torch.zeros(2, 64, 3), torch.zeros(2, 3, 64), torch.zeros(2, 7)))
    with pytest.raises(ValueError, match="augment=False"):
        TrainBatchBuilder(2, dataset="kitti360", npoints=64, augment=False).build(sweeps, lengths, td, aug=torch.zeros(2, 6))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        bld.build(sweeps, lengths, td)                                         # everything right but the device
    with pytest.raises(RuntimeError, match="nothing built yet"):
        bld.indices()
    with pytest.raises(ValueError, match="no calibration"):
        bld.set_calibration(VELO_TO_CAM)
    bld.set_step(41)
    assert bld.step_index() == 41


def test_pad_pairs():
    a, b = np.ones((5, 4), np.float32), 2 * np.ones((3, 4), np.float32)
    sweeps, lengths = pad_pairs([(a, b), (b, a)], capacity=8)
    assert sweeps.shape == (2, 2, 8, 4) and lengths.tolist() == [[5, 3], [3, 5]]
    assert sweeps[0, 1, :3].eq(2).all() and sweeps[0, 1, 3:].eq(0).all()
    with pytest.raises(ValueError, match="does not fit"):
        pad_pairs([(a, b)], capacity=4)


def test_new_launchers_are_declared_with_the_bound_arity():
    text = open(os.path.join(ROOT, "include", "pwclo_ops.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("train_batch_pose_kernel_wrapper", "train_batch_sample_kernel_wrapper"):
        m = re.search(r"\bvoid\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, "%s is not declared in include/pwclo_ops.h" % name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][0]), name
        assert _lib.SIGNATURES[name][1] is None
    from pwclonet_pylidarslam_amd import build
    import ctypes
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "train_batch_pose_kernel_wrapper") and hasattr(lib, "train_batch_sample_kernel_wrapper")


def test_row_filters_are_defined_once():
    """The builder shares the filters' row bodies with warp.hip through csrc/rows.hpp: one definition each."""
    csrc = os.path.join(ROOT, "pwclonet_pylidarslam_amd", "csrc")
    defs = {"kitti_row": [], "kitti360_row": []}
    for f in sorted(os.listdir(csrc)):
        src = open(os.path.join(csrc, f)).read()
        for name in defs:
            if re.search(r"\bbool\s+%s\s*\(" % name, src):
                defs[name].append(f)
    assert defs == {"kitti_row": ["rows.hpp"], "kitti360_row": ["rows.hpp"]}, defs
