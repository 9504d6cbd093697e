"""The evaluation kernels (csrc/odometry_eval.hip over csrc/se3.hpp) against the host model of tests/eval_model.py on the tables
of tests/eval_cases.py.  The model is float64 NumPy in the kernels' own order and association, so transforms, trajectories,
distances, ``valid``, ``first``, ``L``, ``speed`` and ``t_err`` are expected bit for bit (the device's float64 division and
``sqrt`` are correctly rounded); ``r_err`` passes through the device ``acos``, which is not specified as correctly rounded: its
argument is bit-identical, so the only difference is the function's own error, and 4 ulp are allowed (the largest seen is
printed; DESIGN.md records it).  tests/test_eval_cases_cpu.py proves the tables and the model on the CPU.

Run with ``-s`` for the figures."""
import numpy as np
import pytest
import torch

import eval_cases as EC
import eval_model as EM
from pwclonet_pylidarslam_amd import evaluation as E

pytestmark = pytest.mark.gpu
ACOS_ULPS = 4


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _same_bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    bad = np.nonzero((_bits(got) != _bits(want)).reshape(got.shape[0], -1).any(axis=1))[0]
    assert got.shape == want.shape and len(bad) == 0, (what, bad[:8], got[bad[:2]], want[bad[:2]])


@pytest.mark.parametrize("n", EC.ROWS_N)
def test_rows_to_transforms_bit_for_bit(cuda, n):
    rows, kinds = EC.quat_rows(n)
    dev = torch.from_numpy(rows).to(cuda)
    view = torch.full((n, 4, 7), 7.0, device=cuda)               # the level-1 rows of a (B, 4, 7) tensor, no copy
    view[:, 0, :] = dev
    for invert in (False, True):
        want = EM.rows_to_transforms(rows, invert)
        assert np.isfinite(want).all()
        for name, src in (("contiguous", dev), ("view", view[:, 0, :])):
            got = E.rows_to_transforms(src, invert=invert)
            assert got.shape == (n, 4, 4) and got.dtype == torch.float64
            _same_bits(got, want, (name, invert, kinds[:8]))


def test_accumulate_and_distances_bit_for_bit(cuda):
    """All sequences of SCAN_LENGTHS in one launch of each kernel; frames no sequence owns do not exist (the lengths add up),
    so every output element is compared."""
    T = EC.scan_transforms()
    got = E.accumulate(torch.from_numpy(T).to(cuda), EC.SCAN_LENGTHS)
    _same_bits(got, EM.accumulate(T, EC.SCAN_LENGTHS), "accumulate")
    poses = EC.scan_poses()
    dist = E.trajectory_distances(torch.from_numpy(poses).to(cuda), EC.SCAN_LENGTHS)
    want = EM.distances(poses, EC.SCAN_LENGTHS)
    _same_bits(dist, want, "distances")
    starts = EM.starts(EC.SCAN_LENGTHS)
    assert all(want[starts[s]] == 0.0 for s, n in enumerate(EC.SCAN_LENGTHS) if n)
    # one sequence alone (the `lengths=None` form) gives the same bits as inside the launch
    lo, hi = starts[EC.STILL_SEQ], starts[EC.STILL_SEQ + 1]
    _same_bits(E.trajectory_distances(torch.from_numpy(poses[lo:hi].copy()).to(cuda)), want[lo:hi], "one sequence")


@pytest.mark.parametrize("case", EC.ERROR_CASES, ids=lambda c: "%s-%s-step%d" % c)
def test_sequence_errors_edges(cuda, case):
    world, result, step = case
    gt, res, dist = EC.error_inputs(world, result)
    detail = []
    want, want_valid = EM.sequence_errors(gt, res, dist, EC.ERROR_LENGTHS, EC.SEGMENTS, step, detail=detail)
    err, valid, slot_start = E.sequence_errors(torch.from_numpy(gt).to(cuda), torch.from_numpy(res).to(cuda),
                                               torch.from_numpy(dist).to(cuda), EC.ERROR_LENGTHS, EC.SEGMENTS, step)
    assert slot_start == list(EM.starts(EM.slot_counts(EC.ERROR_LENGTHS, len(EC.SEGMENTS), step)))
    got = err.cpu().numpy()
    assert got.shape == want.shape and not np.isnan(got).any()
    assert np.array_equal(valid.cpu().numpy().astype(np.int32), want_valid)
    _same_bits(got[:, [0, 3, 4]], want[:, [0, 3, 4]], "first, L, speed")
    # t_err: bit for bit -- the device sqrt is correctly rounded; were it not, this assertion is where it shows
    t_ulps = EM.ulps(got[:, 2], want[:, 2])
    assert t_ulps.max() == 0, ("t_err ulps", t_ulps.max(), np.nonzero(t_ulps)[0][:8])
    r_ulps = EM.ulps(got[:, 1], want[:, 1])
    print("\n%s %s step %d: %d slots, %d valid; r_err: largest difference %d ulp, %d slots differ; t_err: 0 ulp"
          % (world, result, step, len(got), int(want_valid.sum()), r_ulps.max(), int((r_ulps > 0).sum())))
    assert r_ulps.max() <= ACOS_ULPS, (r_ulps.max(), np.nonzero(r_ulps > ACOS_ULPS)[0][:8])
    if result == "same":
        assert got[want_valid != 0, 1].max() < 1e-7 and (got[:, 2] < 1e-12).all()
    if world == "metre":
        assert (got[:, 1] == 0.0).all()                           # res = gt and the drift: r_err exactly 0, never NaN
    if case == ("turning", "same", 1):
        assert sum(1 for d in detail if d[4] > 1.0) > 0           # the clamp was needed
