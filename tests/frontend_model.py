"""Host model of the raw-frame front end (csrc/rows.hpp, csrc/warp.hip) -- TEST INFRASTRUCTURE, NumPy only.

The library is built with ``-ffp-contract=off``, so every function here is written in the kernel's source order and its result
is expected bit for bit (all comparisons on the int32 view of the fp32 words):

  kitti_row            rows.hpp kitti_row: float64, ((t0 x + t1 y) + t2 z) + t3 per output row, strict comparisons on the
                       float64 values, coordinates rounded to fp32 once;
  kitti360_row         rows.hpp kitti360_row: fp32 comparisons against float32(ground_z) / float32(near), xyz = columns 0..2;
  compact_buffer       compact_frames_scan_kernel and the second half of sweep_filter_compact_kernel: stable compaction of
                       the rows with keep != 0, kept row p written iff p < cap, count = min(kept, cap);
  compact              (xyz words, keep, cap) -> (packed, count): the specification, zero rows past count;
  sweep_filter_compact sweep_filter_compact_kernel for one stream of an (S, R, 4) batch: length clamped to [0, R], no row
                       past it read, zero rows up to cap written by the kernel itself;
  ingest_*             the three input adapters: index arithmetic only.

A NaN that the KITTI arithmetic PRODUCES (0 x inf, inf - inf, or a NaN input carried through five float64 operations) has a
payload and sign that IEEE 754 leaves to the implementation; ``canon_nan`` maps every NaN word to one quiet NaN, and the
KITTI coordinates are compared after it.  Everything that is COPIED (kitti360 coordinates, compaction, ingest) keeps its bits.

``fault=`` plants one named way in which a kernel could be wrong (FAULTS); tests/test_frontend_cases_cpu.py shows that the
case table tells each of them from the model.  ``wave_layout`` is the kernels' own arithmetic for the 16 waves of a
workgroup; only the fault "unstable" and the coverage proof use it.
"""
import numpy as np

GROUND_Y = 1.1                       # rows.hpp: ground = y' > 1.1
NEAR_XZ = 30.0                       # rows.hpp: |x'| < 30 and |z'| < 30
KITTI360_GROUND_Z = -(1.73 - 0.3)    # preprocess.KITTI360_GROUND_Z
QNAN = np.int32(0x7FC00000)

KITTI_FAULTS = ("kitti_y_ge", "kitti_x_le", "kitti_x_ge", "kitti_z_le", "kitti_z_ge")
KITTI360_FAULTS = ("k360_z_le", "k360_x_le", "k360_x_ge", "k360_y_le", "k360_y_ge")
COMPACT_FAULTS = ("keep_eq_1", "p_le_cap", "count_unclipped", "unstable")
SWEEP_FAULTS = ("fill_from_count_plus_1", "length_neg_unclamped", "length_long_unclamped")
FAULTS = KITTI_FAULTS + KITTI360_FAULTS + COMPACT_FAULTS + SWEEP_FAULTS


def canon_nan(words):
    """int32 words of fp32 values -> the same with every NaN replaced by one quiet NaN."""
    w = np.array(words, dtype=np.int32, copy=True)
    w[np.isnan(w.view(np.float32))] = QNAN
    return w


def wave_layout(n):
    """-> (per_wave, [(i0, i1)] of the 16 waves) as both compaction kernels compute them; i1 < i0 for a wave past the end."""
    per_wave = ((n + 15) // 16 + 63) // 64 * 64
    return per_wave, [(w * per_wave, min(n, w * per_wave + per_wave)) for w in range(16)]


def kitti_row(points, tr, fault=None):
    """points (n, 4) f32, tr 12 float64 (rows of the 3x4 calibration) -> (xyz (n, 3) int32 words, keep (n,) bool)."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 4)
    t = np.asarray(tr, dtype=np.float64).reshape(-1)[:12]
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        o = [((t[4 * r + 0] * x + t[4 * r + 1] * y) + t[4 * r + 2] * z) + t[4 * r + 3] for r in range(3)]
        ground = o[1] >= GROUND_Y if fault == "kitti_y_ge" else o[1] > GROUND_Y
        x_hi = o[0] <= NEAR_XZ if fault == "kitti_x_le" else o[0] < NEAR_XZ
        x_lo = o[0] >= -NEAR_XZ if fault == "kitti_x_ge" else o[0] > -NEAR_XZ
        z_hi = o[2] <= NEAR_XZ if fault == "kitti_z_le" else o[2] < NEAR_XZ
        z_lo = o[2] >= -NEAR_XZ if fault == "kitti_z_ge" else o[2] > -NEAR_XZ
        xyz = np.stack(o, axis=1).astype(np.float32)
    return np.ascontiguousarray(xyz).view(np.int32), ~ground & ((x_hi & x_lo) & (z_hi & z_lo))


def kitti360_row(points, ground_z, near, fault=None):
    """points (n, 4) f32 -> (xyz (n, 3) int32 words: columns 0..2 as they are, keep (n,) bool)."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 4)
    gz, nr = np.float32(ground_z), np.float32(near)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        ground = z <= gz if fault == "k360_z_le" else z < gz
        x_hi = x <= nr if fault == "k360_x_le" else x < nr
        x_lo = x >= -nr if fault == "k360_x_ge" else x > -nr
        y_hi = y <= nr if fault == "k360_y_le" else y < nr
        y_lo = y >= -nr if fault == "k360_y_ge" else y > -nr
    return np.ascontiguousarray(p[:, :3]).view(np.int32), ~ground & ((x_hi & x_lo) & (y_hi & y_lo))


def compact_buffer(words, keep, cap, buffer, zero_fill, fault=None):
    """The compaction on a caller's buffer: ``buffer`` (rows >= cap, 3) int32 is what the output memory holds before the
    launch (rows past cap are the guard); kept row number p goes to buffer[p] iff p < cap; ``zero_fill``: rows
    [count, cap) are zeroed (the sweep kernel), else left alone (the scan kernel).  -> (buffer after, count)."""
    words = np.asarray(words, dtype=np.int32).reshape(-1, 3)
    keep = np.asarray(keep)
    n = words.shape[0]
    out = np.array(buffer, dtype=np.int32, copy=True)
    assert keep.shape == (n,) and out.ndim == 2 and out.shape[1] == 3 and out.shape[0] >= cap + 1 > 1
    kept = np.nonzero(keep == 1 if fault == "keep_eq_1" else keep != 0)[0]
    if fault == "unstable":                                   # wave bases summed from the far end: ranges in reverse order
        ranges = [kept[(kept >= i0) & (kept < i1)] for i0, i1 in wave_layout(n)[1] if i0 < i1]
        kept = np.concatenate(ranges[::-1]) if ranges else kept
    limit = cap + 1 if fault == "p_le_cap" else cap
    m = min(len(kept), limit)
    out[:m] = words[kept[:m]]
    count = len(kept) if fault == "count_unclipped" else min(len(kept), cap)
    if zero_fill:
        out[min(count, cap) + (1 if fault == "fill_from_count_plus_1" else 0):cap] = 0
    return out, count


def compact(words, keep, cap):
    """(xyz words (n, 3) int32, keep (n,) integers, cap) -> (packed (cap, 3) int32, count): the rows with keep != 0 in frame
    order, at most cap of them, zero rows past count."""
    out, count = compact_buffer(words, keep, cap, np.zeros((cap + 1, 3), np.int32), True)
    return out[:cap], count


def sweep_filter_compact(sweeps, s, length, cap, buffer, dataset, tr=None, ground_z=KITTI360_GROUND_Z, near=NEAR_XZ,
                         fault=None):
    """Stream s of sweeps (S, R, 4) f32 through sweep_filter_compact_kernel: n = min(max(length, 0), R), only rows [0, n) of
    the stream are read.  ``tr``: this stream's 12 float64.  -> (buffer after, count, xyz words (n, 3), keep (n,)).  The
    unclamped faults read what a kernel without the clamp would: the stream's rows [:length] with Python's negative index
    rule, or on into the next stream's rows."""
    S, R, _ = sweeps.shape
    n = min(max(int(length), 0), R)
    rows = sweeps[s, :n]
    if fault == "length_neg_unclamped" and length < 0:
        rows = sweeps[s, :length]
    if fault == "length_long_unclamped" and length > R:
        rows = sweeps.reshape(-1, 4)[s * R:s * R + length]
    if dataset == "kitti":
        words, keep = kitti_row(rows, tr, fault)
    else:
        words, keep = kitti360_row(rows, ground_z, near, fault)
    out, count = compact_buffer(words, keep.astype(np.int32), cap, buffer, True, fault)
    return out, count, words, keep


def ingest_pairs(f1, f2):
    """Two channel-major batches (B, 3, n) -> one point-major (2B, n, 3), frame 1 first.  Any dtype: words are copied."""
    return np.ascontiguousarray(np.concatenate((f1, f2), axis=0).transpose(0, 2, 1))


def ingest_frames(f1, f2, n):
    """Two point-major batches (B, n_total, c) -> (2B, n, 3): the first n rows and the first 3 channels, frame 1 first."""
    return np.ascontiguousarray(np.concatenate((f1, f2), axis=0)[:, :n, :3])


def ingest_sequence(frames, n):
    """(T, n_total, c) -> (T, n, 3), frame order kept."""
    return np.ascontiguousarray(frames[:, :n, :3])
