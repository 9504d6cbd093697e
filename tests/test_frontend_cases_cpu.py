"""tests/frontend_model.py and tests/frontend_cases.py on the CPU: the model is the dataset code, the tables of
tests/test_gpu_frontend.py reach every class of the compaction kernels' arithmetic, and every planted fault of the model is
told from it by at least one row of the tables.

Run with ``-s`` for the figures."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frontend_cases as FC                                                      # noqa: E402
import frontend_model as FM                                                      # noqa: E402
import gather_cases as GC                                                        # noqa: E402
from oracle import preprocess as OP                                              # noqa: E402


def _ulp32(a_words, b_f32):
    return np.abs(a_words.astype(np.int64) - np.ascontiguousarray(b_f32).view(np.int32).astype(np.int64))


def test_model_is_the_dataset_code_on_random_rows():
    """Against oracle/preprocess.py (a BLAS matmul, another summation order): coordinates within 1 fp32 ulp, the mask
    identical on every row that is not within 1e-9 of a threshold; KITTI-360 (no arithmetic) bit for bit."""
    rng = np.random.default_rng(3)
    n = 20000
    pts = np.concatenate([rng.uniform(-70, 70, (n, 2)), rng.uniform(-3, 2, (n, 1)), rng.uniform(0, 1, (n, 1))],
                         axis=1).astype(np.float32)
    q, keep = OP.transform_filter(pts, FC.GENERAL_TR)
    words, k = FM.kitti_row(pts, FC.GENERAL_TR)
    ulp = _ulp32(words, q.astype(np.float32))
    away = (np.abs(np.abs(q[:, [0, 2]]) - 30).min(axis=1) > 1e-9) & (np.abs(q[:, 1] - 1.1) > 1e-9)
    print("\nkitti_row vs BLAS order: max %d ulp, %d of %d words differ; %d rows near a threshold"
          % (ulp.max(), (ulp > 0).sum(), ulp.size, (~away).sum()))
    assert ulp.max() <= 1 and away.mean() > 0.99
    assert np.array_equal(k[away], keep[away]) and 0.05 < k.mean() < 0.95
    for near in (30.0, 35.0):
        p360, k360 = OP.kitti360_filter(pts, near)
        w, k2 = FM.kitti360_row(pts, FM.KITTI360_GROUND_Z, near)
        assert np.array_equal(w, np.ascontiguousarray(p360).view(np.int32)) and np.array_equal(k2, k360)


def test_threshold_rows_sit_where_the_table_says():
    """Under the permutation the outputs are the inputs; rows on a threshold and on both fp32 neighbours exist for every
    comparison, and the "scale" calibration reaches the float64 1.1 itself."""
    rows = FC.filter_rows("kitti", "permute")
    words, keep = FM.kitti_row(rows, FC.PERMUTE_TR)
    out = words.view(np.float32).astype(np.float64)
    finite = np.isfinite(rows[:, :3]).all(axis=1)
    assert np.array_equal(out[finite], rows[finite][:, [1, 2, 0]].astype(np.float64))      # +0 for -0: equal as values
    for col in (0, 2):
        for t in (30.0, -30.0):
            lo, hi = np.nextafter(np.float32(t), np.float32(-np.inf)), np.nextafter(np.float32(t), np.float32(np.inf))
            for v in (lo, np.float32(t), hi):
                at = np.nonzero(finite & (out[:, col] == np.float64(v)))[0]
                assert len(at) and (keep[at] == (abs(np.float64(v)) < 30.0)).all(), (col, v)
    below, above = out[finite, 1][out[finite, 1] < 1.1].max(), out[finite, 1][out[finite, 1] > 1.1].min()
    assert np.float32(below) == below and np.nextafter(np.float32(below), np.float32(np.inf)) == np.float32(above)
    w2, k2 = FM.kitti_row(FC.filter_rows("kitti", "scale"), FC.SCALE_TR)
    y = 1.1 * FC.filter_rows("kitti", "scale")[:, 2].astype(np.float64)
    assert (y == 1.1).sum() >= 3 and k2[y == 1.1].any()
    rows = FC.filter_rows("kitti360")
    gz = np.float32(FC.GROUND_Z)
    _, k360 = FM.kitti360_row(rows, FC.GROUND_Z, FC.NEAR)
    for v, want in ((np.nextafter(gz, np.float32(-np.inf)), False), (gz, True), (np.nextafter(gz, np.float32(np.inf)), True)):
        at = np.nonzero(rows[:, 2] == v)[0]
        assert len(at) and (k360[at] == want).all()
    for col in (0, 1):
        for t in (30.0, -30.0):
            at = np.nonzero(rows[:, col] == np.float32(t))[0]
            assert len(at) and not k360[at].any()
    # every special value in every column, and what the comparisons make of it (NaN compares false both ways)
    for col in range(4):
        for v in FC.SPECIAL_VALUES:
            assert (rows[:, col].view(np.int32) == v.view(np.int32)).any(), (col, v)
    nan_z = np.nonzero(np.isnan(rows[:, 2]))[0]
    assert len(nan_z) and k360[nan_z].all()                       # not "z < ground_z": kept


def test_table_covers_every_layout_class():
    """Enumerated: every (per_wave, non-empty ranges, last 64-step) class a frame of 1 .. 2049 rows can have is in COMPACT_N
    and among the sweep lengths; 1025 is where per_wave jumps and waves 9 .. 15 start past the end."""
    reachable = {FC.layout_class(n) for n in range(1, FC.MAX_N + 1)}
    assert len(reachable) == 16
    assert {FC.layout_class(n) for n in FC.COMPACT_N} == reachable
    assert set(FC.ISSUE_N) <= set(FC.COMPACT_N)
    assert FM.wave_layout(1024)[0] == 64 and FM.wave_layout(1025)[0] == 128
    assert [i0 < i1 for i0, i1 in FM.wave_layout(1025)[1]] == [True] * 9 + [False] * 7
    sweep = [L for row in FC.SWEEP_LENGTHS for L in row]
    assert set(FC.COMPACT_N) <= set(sweep) and {0, -5, FC.SWEEP_R + 9, FC.SWEEP_R} <= set(sweep)
    assert all(len(row) == FC.SWEEP_S for row in FC.SWEEP_LENGTHS)
    for n in FC.COMPACT_N:                                        # the pattern that names the waves hits each range once
        k = FC.keep_pattern("one_per_wave", n, 0)
        assert [int((k[i0:i1] != 0).sum()) for i0, i1 in FM.wave_layout(n)[1] if i0 < i1] == \
            [1] * sum(i0 < i1 for i0, i1 in FM.wave_layout(n)[1])
    words = {int(w) for n in (64, 1025) for w in FC.keep_pattern("all", n, 0)}
    assert words == {1, 2, -1, FC.INT_MIN}


def test_compaction_model_is_boolean_indexing():
    for n, b, pattern, fill in FC.compact_cases():
        if b != 3 or fill != "identity":
            continue
        keep, xyz = FC.compact_keep(pattern, b, n), FC.xyz_fill(fill, b, n, n)
        for f in range(b):
            kept = xyz[f][keep[f] != 0]
            for cap in FC.caps_for([len(kept)], n):
                packed, count = FM.compact(xyz[f], keep[f], cap)
                assert count == min(len(kept), cap) and packed.shape == (cap, 3)
                assert np.array_equal(packed[:count], kept[:count]) and not packed[count:].any()


def _compact_differs(fault):
    for n, b, pattern, fill in FC.compact_cases():
        keep, xyz = FC.compact_keep(pattern, b, n), FC.xyz_fill(fill, b, n, n)
        counts = [int((keep[f] != 0).sum()) for f in range(b)]
        for cap in FC.caps_for(counts, n):
            for f in range(b):
                buf = FC.guard_buffer(cap, 2)
                if not _same(FM.compact_buffer(xyz[f], keep[f], cap, buf, False),
                             FM.compact_buffer(xyz[f], keep[f], cap, buf, False, fault)):
                    return (n, b, pattern, fill, cap, f)
    return None


def _same(a, b):
    return a[1] == b[1] and np.array_equal(a[0], b[0])


def _sweep_differs(fault):
    for dataset in FC.DATASETS:
        for li, lengths in enumerate(FC.SWEEP_LENGTHS):
            batch = FC.sweep_batch(dataset, lengths, "live", 50 + li)
            for cap in FC.caps_for(FC.sweep_counts(dataset, batch, lengths), FC.SWEEP_R):
                bufs = [FC.guard_buffer(cap, 2, FC.SWEEP_PREFILL) for _ in lengths]
                good, bad = FC.sweep_model(dataset, batch, lengths, cap, bufs), FC.sweep_model(dataset, batch, lengths, cap, bufs, fault)
                for s in range(FC.SWEEP_S):
                    if good[1][s] != bad[1][s] or not np.array_equal(good[0][s], bad[0][s]):
                        return (dataset, lengths, cap, s)
    return None


def _filter_differs(fault):
    for case in FC.filter_cases():
        pts = FC.filter_input(case)
        (w0, k0), (w1, k1) = FC.filter_model(case, pts), FC.filter_model(case, pts, fault)
        if not np.array_equal(k0, k1):
            return case
    return None


@pytest.mark.parametrize("fault", FM.FAULTS)
def test_every_fault_is_caught(fault):
    if fault in FM.KITTI_FAULTS + FM.KITTI360_FAULTS:
        where = _filter_differs(fault)
        also = _sweep_differs(fault)                              # the sweep kernel has its own instantiation of the rows
        assert also is not None, fault
    elif fault in FM.COMPACT_FAULTS:
        where = _compact_differs(fault)
        assert fault == "keep_eq_1" or _sweep_differs(fault) is not None, fault      # the sweep kernel has no keep words
    else:
        where = _sweep_differs(fault)
    print("\n%s: first caught by %s" % (fault, (where,)))
    assert where is not None, fault


def test_ingest_models_are_the_torch_expressions():
    """The adapters the kernels replace: cat + permute, slice + cat."""
    for n in FC.INGEST_N:
        for b in FC.INGEST_B:
            f1, f2 = GC.fill("bits", b, 3, n, n), GC.fill("identity", b, 3, n, n)
            out = FM.ingest_pairs(f1, f2)
            assert out.shape == (2 * b, n, 3) and out[0, n - 1, 2] == f1[0, 2, n - 1] and out[2 * b - 1, 0, 1] == f2[b - 1, 1, 0]
            for c in FC.INGEST_C:
                for extra in FC.INGEST_EXTRA:
                    g1, g2 = GC.fill("identity", b, n + extra, c, 1), GC.fill("bits", b, n + extra, c, 2)
                    out = FM.ingest_frames(g1, g2, n)
                    assert out.shape == (2 * b, n, 3) and out.flags.c_contiguous
                    assert np.array_equal(out[b:, :, 2], g2[:, :n, 2]) and np.array_equal(out[:b, n - 1], g1[:, n - 1, :3])
                    seq = FM.ingest_sequence(np.concatenate((g1, g2)), n)
                    assert np.array_equal(seq, out)
