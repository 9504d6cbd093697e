"""tests/eval_model.py and tests/eval_cases.py on the CPU: the model's scan association is as good as the plain loop (both
judged against an 80-bit np.longdouble evaluation), the model is the NumPy oracle's evaluation, the tables of
tests/test_gpu_eval_edges.py reach every class of the kernels' arithmetic, and every planted fault is told from the model.

Run with ``-s`` for the figures."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_cases as EC                                                          # noqa: E402
import eval_model as EM                                                          # noqa: E402
from oracle import eval_oracle as EO                                             # noqa: E402
from oracle.gen_eval_golden import synthetic_rows                                # noqa: E402

LD = np.longdouble
MARGIN = 4.0          # the project's margin wherever only the summation order differs
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _per_sequence(lengths):
    lo = 0
    for s, n in enumerate(lengths):
        yield s, n, lo
        lo += n


def _max_rms(err):
    err = np.asarray(err, dtype=np.float64)
    return float(np.abs(err).max()), float(np.sqrt((err * err).mean()))


ACC_MAX_EXCEPTION = (63,)    # see test_scan_association_is_as_good_as_the_plain_loop


def test_scan_association_is_as_good_as_the_plain_loop():
    """Per sequence of SCAN_LENGTHS, both judged against the 80-bit evaluation of the same inputs: the scan's max and RMS
    error are each at most 4 x the plain float64 loop's, for the trajectories and for the distances; for n <= 2 (the same
    operations in the same order) and wherever the plain loop has no error, the scan equals it bit for bit.

    One figure is excepted by name and judged otherwise: the MAX trajectory error of the 63-frame sequence, 3.00e-14 against
    the plain loop's 6.81e-15, a ratio of 4.41 (its RMS ratio is 2.80 and is asserted).  A sequence's maximum is a single
    rounding history, and this plain loop's is a lucky one: the smallest of the nine below, half an ulp of its 63 m.  So the
    max trajectory error of EVERY sequence, this one included, is also held to 4 x a yardstick that does not hinge on one
    history: the median, over the table's inputs and eight more drawn the same way (eval_cases.YARDSTICK_SEEDS, fixed
    beforehand), of the plain loop's max error at that length.  DESIGN.md records the 4.41."""
    assert np.finfo(LD).nmant >= 63                               # the yardstick has 11 more bits than float64
    plain_max = {}
    for seed in EC.YARDSTICK_SEEDS:
        Ts = EM.from_4x4(EC.scan_transforms(seed))
        for s, n, lo in _per_sequence(EC.SCAN_LENGTHS):
            if n:
                err = EM.sequential_accumulate(Ts[lo:lo + n], np.float64) - EM.sequential_accumulate(Ts[lo:lo + n], LD)
                plain_max.setdefault(s, []).append(_max_rms(err)[0])
    T = EC.scan_transforms()
    got = EM.from_4x4(EM.accumulate(T, EC.SCAN_LENGTHS))
    poses = EC.scan_poses()
    dist = EM.distances(poses, EC.SCAN_LENGTHS)
    excepted = []
    for s, n, lo in _per_sequence(EC.SCAN_LENGTHS):
        if n == 0:
            continue
        seq = EM.from_4x4(T[lo:lo + n])
        exact, plain = EM.sequential_accumulate(seq, LD), EM.sequential_accumulate(seq, np.float64)
        p = poses[lo:lo + n, :3, 3]
        d_exact, d_plain = EM.sequential_distances(p, LD), EM.sequential_distances(p, np.float64)
        a_scan, a_plain = _max_rms(got[lo:lo + n] - exact), _max_rms(plain - exact)
        d_scan, d_plain_e = _max_rms(dist[lo:lo + n] - d_exact), _max_rms(d_plain - d_exact)
        yard = float(np.median(plain_max[s]))
        print("\nn=%3d  accumulate max %.2e / %.2e rms %.2e / %.2e, yardstick %.2e;  distances max %.2e / %.2e rms %.2e / %.2e"
              "  (scan / plain)" % ((n,) + tuple(v for pair in zip(a_scan, a_plain) for v in pair) + (yard,)
                                  + tuple(v for pair in zip(d_scan, d_plain_e) for v in pair)))
        if n <= 2:
            assert np.array_equal(got[lo:lo + n], plain) and np.array_equal(dist[lo:lo + n], d_plain)
        assert dist[lo] == 0.0 and plain_max[s][0] == a_plain[0]  # the first yardstick input is the table's
        checks = [("accumulate rms", a_scan[1], a_plain[1]), ("distances max", d_scan[0], d_plain_e[0]),
                  ("distances rms", d_scan[1], d_plain_e[1]), ("accumulate max / yardstick", a_scan[0], yard)]
        if n in ACC_MAX_EXCEPTION:
            excepted.append((n, a_scan[0], a_plain[0]))
        else:
            checks.append(("accumulate max", a_scan[0], a_plain[0]))
        for what, a, b in checks:
            assert a <= MARGIN * b and (b > 0 or a == 0), (what, n, a, b)
    assert [e[0] for e in excepted] == list(ACC_MAX_EXCEPTION)
    for n, a, b in excepted:
        print("\nexcepted by name: accumulate max at n=%d, scan %.2e against plain %.2e = %.2f x" % (n, a, b, a / b))


def test_model_is_the_oracles_evaluation():
    """One golden case (the imported reference's values pin oracle/eval_oracle.py in tests/test_oracle_cpu.py): the model's
    transforms, trajectories, distances and segment errors against the oracle's float64 loops."""
    z = np.load(os.path.join(GOLDEN, "eval_cases.npz"))
    cases = json.loads(str(z["meta"]))["cases"]
    name = "drive_a"                                              # the 900-frame case
    gt_rows, pred_rows = synthetic_rows(**cases[name])
    n = gt_rows.shape[0]
    q = z["quat.q"].astype(np.float32)
    R = EM.rows_to_transforms(np.concatenate((np.zeros((len(q), 3), np.float32), q), axis=1))[:, :3, :3]
    for i in range(len(q)):
        np.testing.assert_allclose(R[i], EO.quat2mat(q[i].astype(np.float64)), rtol=0, atol=1e-15)
    rel = EO.rows_to_relative(pred_rows.astype(np.float64))
    np.testing.assert_allclose(EM.rows_to_transforms(pred_rows, invert=True), np.stack(rel), rtol=0, atol=1e-12)
    ab = {}
    for key, rows in (("gt", gt_rows), ("pred", pred_rows)):
        want = EO.convert_to_absolute({i: m for i, m in enumerate(EO.rows_to_relative(rows.astype(np.float64)))})
        ab[key] = EM.accumulate(EM.rows_to_transforms(rows), [n])
        np.testing.assert_allclose(ab[key], np.stack([want[i] for i in range(n)]), rtol=0, atol=1e-9)
    dist = EM.distances(ab["gt"], [n])
    gt_d, pred_d = ({i: m for i, m in enumerate(ab[k])} for k in ("gt", "pred"))
    np.testing.assert_allclose(dist, EO.trajectory_distances(gt_d), rtol=1e-13, atol=0)
    want = np.array(EO.calc_sequence_errors(gt_d, pred_d)).reshape(-1, 5)
    err, valid = EM.sequence_errors(ab["gt"], ab["pred"], dist, [n], EO.DEFAULT_SEGMENTS, 10)
    got = err[valid != 0]
    print("\n%s: %d frames, %d valid segments of %d slots" % (name, n, len(got), len(err)))
    assert len(want) > 50 and got.shape == want.shape
    assert np.array_equal(got[:, [0, 3]], want[:, [0, 3]])
    np.testing.assert_allclose(got[:, 4], want[:, 4], rtol=1e-15)
    np.testing.assert_allclose(got[:, 1:3], want[:, 1:3], rtol=1e-7, atol=1e-12)
    bad = err[valid == 0]
    assert len(bad) and not bad[:, [1, 2, 4]].any() and (bad[:, 3] > 0).all()


def test_edge_quaternions_are_what_they_claim():
    rows, kinds = EC.quat_rows(257)
    nq = EM.norm2(rows)
    below, above = np.nextafter(1e-8, 0.0), np.nextafter(1e-8, 1.0)
    for kind, want in (("at_1e-8", 1e-8), ("below_1e-8", below), ("above_1e-8", above), ("zero", 0.0)):
        at = [i for i, k in enumerate(kinds) if k == kind]
        assert len(at) > 30 and (nq[at] == want).all(), kind
    assert set(kinds) == set(EC.QUAT_KINDS)
    T = EM.rows_to_transforms(rows)
    for i, kind in enumerate(kinds):
        ident = np.array_equal(T[i, :3, :3], np.eye(3))
        assert ident == (kind in ("zero", "below_1e-8")), kind    # AT 1e-8 the rule is strict: a rotation
        assert np.array_equal(T[i, :3, 3], rows[i, :3].astype(np.float64)) and np.isfinite(T[i]).all()
    for kind, scale in (("norm0.1", 0.1), ("norm10", 10.0)):
        at = [i for i, k in enumerate(kinds) if k == kind]
        np.testing.assert_allclose(np.sqrt(nq[at]), scale, rtol=1e-6)
        RtR = np.einsum("nij,nik->njk", T[at, :3, :3], T[at, :3, :3])
        np.testing.assert_allclose(RtR, np.tile(np.eye(3), (len(at), 1, 1)), atol=1e-14)       # still a rotation


def test_tables_reach_every_class():
    for lengths in (EC.SCAN_LENGTHS, EC.ERROR_LENGTHS):
        assert lengths[0] == 0 and lengths[-1] == 0 and 0 in lengths[1:-1]          # empty first, in the middle, last
    chunks = {EM.lane_chunks(n)[0] for n in EC.SCAN_LENGTHS if n}
    assert chunks == {1, 2, 3} and {1, 2, 63, 64, 65, 127, 128, 129} <= set(EC.SCAN_LENGTHS)
    for chunk in (1, 2):                                          # lanes that own nothing, at both chunk sizes
        assert any(n and EM.lane_chunks(n)[0] == chunk and (EM.lane_chunks(n)[1] == EM.lane_chunks(n)[2]).any()
                   for n in EC.SCAN_LENGTHS)
    assert EC.SCAN_LENGTHS[EC.STILL_SEQ] > EC.STILL[1]
    d = EM.distances(EC.scan_poses(), EC.SCAN_LENGTHS)
    lo = sum(EC.SCAN_LENGTHS[:EC.STILL_SEQ])
    still = np.diff(d[lo + EC.STILL[0] - 1:lo + EC.STILL[1]])
    # the stationary stretch: every step is exactly 0, so distances tie inside a lane's chunk; from one lane to the next the
    # prefix comes from another association of the same sum and may sit one ulp higher OR LOWER (the scan's
    # distances are non-decreasing only up to an ulp)
    print("\nstationary stretch: %d ties, %d steps up, %d steps down by at most %.1e" % ((still == 0).sum(), (still > 0).sum(),
                                                                                      (still < 0).sum(), np.abs(still).max()))
    assert (still == 0).sum() >= 10 and np.abs(still).max() <= np.spacing(d[lo + EC.STILL[0]])
    totals = {step: sum(EM.slot_counts(EC.ERROR_LENGTHS, len(EC.SEGMENTS), step)) for step in EC.STEPS}
    assert totals[1] > 256 > totals[4] and all(any(n % step for n in EC.ERROR_LENGTHS) for step in (4, 10))
    gt, res, dist = EC.error_inputs("metre", "same")
    assert np.array_equal(dist, np.round(dist)) and (np.diff(dist)[np.diff(dist) >= 0] == 0).any()
    seen = {"on_distance": 0, "ties": 0, "invalid": 0, "above_one": 0}
    for world, result, step in EC.ERROR_CASES:
        gt, res, dist = EC.error_inputs(world, result)
        detail = []
        err, valid = EM.sequence_errors(gt, res, dist, EC.ERROR_LENGTHS, EC.SEGMENTS, step, detail=detail)
        assert not np.isnan(err).any()
        seen["invalid"] += int((valid == 0).sum())
        starts = EM.starts(EC.ERROR_LENGTHS)
        for slot, s, first, last, tr, r_err, t_err in detail:
            ds = dist[starts[s]:starts[s + 1]]
            L = err[slot, 3]
            seen["on_distance"] += int(ds[last - 1] == ds[first] + L)                # strict: the frame ON it is not the last
            seen["ties"] += int(last + 1 < len(ds) and ds[last + 1] == ds[last]) + int(ds[last - 1] == ds[first] + L and last >= 2 and ds[last - 2] == ds[last - 1])
            seen["above_one"] += int(tr > 1.0)
            if world == "metre":
                assert r_err == 0.0 and t_err == (EC.DRIFT - 1.0) * (ds[last] - ds[first]) * (result == "drift")
            if result == "same":
                assert r_err < 1e-7 and t_err < 1e-12
    print("\nslots per step %s; %s" % (totals, seen))
    assert all(v > 0 for v in seen.values()), seen


def _rows_differ(fault):
    for n in EC.ROWS_N:
        rows, kinds = EC.quat_rows(n)
        for invert in (False, True):
            a, b = EM.rows_to_transforms(rows, invert), EM.rows_to_transforms(rows, invert, fault)
            if not np.array_equal(a, b):
                return (n, invert, kinds[int(np.nonzero((a != b).any(axis=(1, 2)))[0][0])])
    return None


def _errors_differ(fault):
    for world, result, step in EC.ERROR_CASES:
        gt, res, dist = EC.error_inputs(world, result)
        a = EM.sequence_errors(gt, res, dist, EC.ERROR_LENGTHS, EC.SEGMENTS, step)
        b = EM.sequence_errors(gt, res, dist, EC.ERROR_LENGTHS, EC.SEGMENTS, step, fault)
        if not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])):
            return (world, result, step)
    return None


@pytest.mark.parametrize("fault", EM.FAULTS)
def test_every_fault_is_caught(fault):
    if fault in ("identity_le", "invert_ignored"):
        where = _rows_differ(fault)
    elif fault == "first_distance_nonzero":
        poses = EC.scan_poses()
        same = np.array_equal(EM.distances(poses, EC.SCAN_LENGTHS), EM.distances(poses, EC.SCAN_LENGTHS, fault))
        where = None if same else "scan lengths"
    else:
        where = _errors_differ(fault)
    print("\n%s: first caught by %s" % (fault, (where,)))
    assert where is not None, fault
