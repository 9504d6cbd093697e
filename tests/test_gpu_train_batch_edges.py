"""GPU tests of csrc/train_batch.hip at its edges (run with ``-m gpu``): the tables of tests/train_batch_cases.py through
``TrainBatchBuilder.build`` against the NumPy host model (tests/train_batch_model.py).  tests/test_train_batch_cases_cpu.py
shows what each table reaches and which fault of the kernel it would catch: the tie pass, P > npoints, the count and row-count
boundaries, device lengths with the ``n == 0`` rule, every quaternion / Euler branch, and B > 256.

Selection (indices, survivor counts) and every unaugmented coordinate are compared BIT FOR BIT.  What passes through libm in
fp64 on both sides keeps the bounds of tests/test_gpu_train_batch.py: drawn parameters and moved coordinates 1 fp32 ulp,
``t_gt`` 1e-12 relative, quaternion 2^-23, translation 1 ulp of max(|t|, 1).  The three outputs are written through ``out=``
into leading views of larger buffers whose tails must stay untouched."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_batch_cases as TC                                                # noqa: E402
import train_batch_model as model                                             # noqa: E402

from pwclonet_pylidarslam_amd.batches import TrainBatchBuilder                # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL, TAIL = 0x5A5A5A5A, 64


@pytest.fixture(scope="module", autouse=True)
def first_build_is_eager(cuda):
    """the launcher raises the kernel's dynamic-LDS limit on its first call."""
    bld = TrainBatchBuilder(1, dataset="kitti360", npoints=8, capacity=64)
    bld.build(torch.from_numpy(TC.raw_rows(64, 0)).to(cuda).expand(1, 2, 64, 4).contiguous(), [[64, 64]],
              torch.eye(4, dtype=torch.float64)[None])
    torch.cuda.synchronize()


def _ulps(a, b):
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def _guarded(shape, cuda):
    """A float32 tensor of ``shape`` that is the head of a larger buffer of sentinel words -> (tensor, whole buffer)."""
    size = int(np.prod(shape))
    flat = torch.full((size + TAIL,), SENTINEL, dtype=torch.int32, device=cuda)
    return flat[:size].view(torch.float32).view(shape), flat


def _words(x):
    return np.ascontiguousarray(x).view(np.int32)


class _Run:
    def __init__(self, cuda, case, arrays):
        B, m = len(case["lengths"]), case["npoints"]
        self.case, self.cuda = case, cuda
        self.bld = TrainBatchBuilder(B, dataset=case["dataset"], npoints=m, capacity=case["R"], augment=case["mode"] != 0,
                                     seed=case["seed"], tr=arrays["tr"])
        self.sweeps = torch.from_numpy(arrays["sweeps"]).to(cuda)
        lengths = torch.from_numpy(arrays["lengths"].astype(np.int32))
        self.lengths = lengths.to(cuda) if case["device_lengths"] else lengths
        self.t_diff = torch.from_numpy(arrays["t_diff"])
        self.aug = torch.from_numpy(arrays["aug"]).to(cuda) if case["mode"] == 2 else None
        self.out, self.flats = zip(*[_guarded(s, cuda) for s in ((B, 3, m), (B, 3, m), (B, 7))])

    def build(self):
        """One build at the case's step -> the outputs as NumPy arrays; the tails behind the three outputs are intact."""
        self.bld.set_step(self.case["step"])
        x1, x2, gt = self.bld.build(self.sweeps, self.lengths, self.t_diff, out=self.out, aug=self.aug)
        torch.cuda.synchronize()
        assert x1 is self.out[0] and x2 is self.out[1] and gt is self.out[2]
        for flat in self.flats:
            assert bool((flat[-TAIL:] == SENTINEL).all())
        b = self.bld
        return dict(xyz_f1=x1.cpu().numpy(), xyz_f2=x2.cpu().numpy(), gt=gt.cpu().numpy(), indices=b.indices().cpu().numpy(),
                    counts=b.survivor_counts().cpu().numpy(), aug=b.aug_params().cpu().numpy(), t_gt=b.t_gt().cpu().numpy())


def _same_bits(a, b):
    return all(np.array_equal(_words(a[k]) if a[k].dtype == np.float32 else a[k].view(np.int64) if a[k].dtype == np.float64
                              else a[k], _words(b[k]) if b[k].dtype == np.float32 else b[k].view(np.int64)
                              if b[k].dtype == np.float64 else b[k]) for k in a)


def _check(case, arrays, got):
    """``got`` against the host model, to the bounds named in the module docstring."""
    B, mode, ds = len(case["lengths"]), case["mode"], case["dataset"]
    if mode == 1:                                          # the drawn parameters, then the model with the DEVICE's
        drawn = np.stack([model.draw_aug(b, case["step"], case["seed"]) for b in range(B)])
        d = _ulps(got["aug"], drawn)
        print("aug_params: max %d ulp from the host model" % d.max())
        assert d.max() <= 1
        ref = TC.expected(case, arrays, aug=got["aug"])
    else:
        ref = TC.expected(case, arrays)
        assert np.array_equal(_words(got["aug"]), _words(ref["aug"]))          # given ones untouched; zeros without augmentation

    assert np.array_equal(got["counts"], ref["counts"]), (got["counts"], ref["counts"])
    bad = np.nonzero((got["indices"] != ref["indices"]).any(axis=1))[0]
    assert len(bad) == 0, (bad, got["indices"][bad[0]], ref["indices"][bad[0]])

    plain, moved = ("xyz_f2", "xyz_f1") if ds == "kitti" else ("xyz_f1", "xyz_f2")
    assert np.array_equal(_words(got[plain]), _words(ref[plain]))
    if mode == 0:
        assert np.array_equal(_words(got[moved]), _words(ref[moved]))
        assert np.array_equal(got["t_gt"].view(np.int64), arrays["t_diff"].view(np.int64))      # T_diff itself
    else:
        d = _ulps(got[moved], ref[moved])
        print("moved coordinates: max %d ulp" % d.max())
        assert d.max() <= 1
    rel = np.abs(got["t_gt"] - ref["t_gt"]).reshape(B, -1).max(axis=1) / np.abs(ref["t_gt"]).reshape(B, -1).max(axis=1)
    print("t_gt: max relative difference %.2e" % rel.max())
    assert rel.max() <= 1e-12
    g = got["gt"]
    dq = np.abs(g[:, 3:].astype(np.float64) - ref["gt"][:, 3:]).max(axis=1)
    tscale = np.maximum(np.abs(ref["gt"][:, :3]).max(axis=1), 1.0).astype(np.float32)
    dt = np.abs(g[:, :3].astype(np.float64) - ref["gt"][:, :3]).max(axis=1) / np.spacing(tscale)
    print("gt: quaternion max abs difference %.2e (pair %d), translation %.2f ulp of max(|t|, 1)" % (dq.max(), dq.argmax(), dt.max()))
    assert dq.max() <= 2.0 ** -23 and dt.max() <= 1.0, (dq.argmax(), g[dq.argmax()], ref["gt"][dq.argmax()])

    for b in range(B):                                     # an empty frame: index -1, +0.0 words, count 0
        if case["device_lengths"] and min(max(v, 0) for v in case["lengths"][b]) == 0:
            assert (got["indices"][2 * b:2 * b + 2] == -1).all() and not got["counts"][2 * b:2 * b + 2].any()
            assert not _words(got["xyz_f1"][b]).any() and not _words(got["xyz_f2"][b]).any()
    return ref


@pytest.mark.parametrize("case", TC.selection_cases(), ids=lambda c: c["name"])
def test_selection_tables(cuda, case):
    arrays = TC.materialise(case)
    run = _Run(cuda, case, arrays)
    got = run.build()
    ref = _check(case, arrays, got)
    if case["table"] == "device_lengths":
        assert (got["indices"][:4] == -1).all() and got["counts"].tolist() == ref["counts"].tolist()
    if case["table"] == "ties":
        cloud = TC.COLLISIONS[case["key"]]["cloud"]
        rows = got["indices"][cloud].tolist()
        assert all(r in rows for r in case["take"]) and not any(r in rows for r in case["leave"])
    if case["table"] in ("ties", "padding"):               # LDS slots are handed out in arrival order; the sort hides it
        assert _same_bits(got, run.build())


@pytest.mark.parametrize("case", TC.pose_cases() + TC.wide_cases(), ids=lambda c: c["name"])
def test_pose_tables(cuda, case):
    arrays = TC.materialise(case)
    got = _Run(cuda, case, arrays).build()
    _check(case, arrays, got)
    assert np.abs(np.linalg.norm(got["gt"][:, 3:], axis=1) - 1).max() < 1e-6
    if case["table"] == "quat" and case["mode"] == 0 and case["dataset"] == "kitti360":
        q = dict(zip(case["names"], got["gt"][:, 3:]))
        assert np.abs(q["third_turn"] - np.array([0.5, 0.5, 0.5, 0.5])).max() <= 2.0 ** -23
        assert np.abs(q["third_turn_back"] - np.array([-0.5, 0.5, 0.5, 0.5])).max() <= 2.0 ** -23
