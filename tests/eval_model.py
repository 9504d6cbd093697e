"""Host model of the evaluation kernels (csrc/odometry_eval.hip over csrc/se3.hpp) -- TEST INFRASTRUCTURE, NumPy float64.

Every function is the kernel's expression in the kernel's order (the library is built with ``-ffp-contract=off``; float64
``+ - * /`` and ``sqrt`` are correctly rounded on both sides), so everything but ``acos`` is expected bit for bit:

  pose_row_to_se3, se3_mul, se3_inv   se3.hpp, on (..., 12) arrays (rows 0..2 of a transform), broadcasting;
  rows_to_transforms                  odom_rows_to_transforms_kernel -> (n, 4, 4);
  accumulate, distances               the two wave scans in THEIR association: lane l of 64 owns the chunk
                                      [l chunk, (l + 1) chunk) with chunk = ceil(n / 64), multiplies / sums it from the
                                      identity / 0, the 64 lane values go through a 6-step Hillis-Steele scan
                                      (``incl = up (x) incl`` for lane >= d, d = 1, 2, .. 32), and every lane replays its
                                      chunk from the exclusive prefix;
  sequence_errors                     odom_sequence_errors_kernel slot by slot: owner search, strict upper-bound search for
                                      the last frame, the invalid row [first, 0, 0, L, 0], the clamped ``acos``.

``sequential_*`` are the plain loops the scans re-associate, in any float type (np.longdouble for the CPU test's yardstick).
``fault=`` plants one named way in which a kernel could be wrong (FAULTS).
"""
import numpy as np

FAULTS = ("search_ge", "last_off_by_one", "owner_no_empty_skip", "no_acos_clamp", "identity_le", "invert_ignored",
          "first_distance_nonzero")
IDENTITY = np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0])
IDENTITY_NORM2 = 1e-8                       # se3.hpp: identity rotation below it


def se3_mul(a, b):
    """c = a . b: s = (a[i0] b[0j] + a[i1] b[1j]) + a[i2] b[2j], and ``s += a[i3]`` for the translation column."""
    a, b = np.broadcast_arrays(a, b)
    c = np.empty(a.shape, dtype=a.dtype)
    for i in range(3):
        for j in range(4):
            s = (a[..., 4 * i] * b[..., j] + a[..., 4 * i + 1] * b[..., 4 + j]) + a[..., 4 * i + 2] * b[..., 8 + j]
            c[..., 4 * i + j] = s + a[..., 4 * i + 3] if j == 3 else s
    return c


def se3_inv(a):
    a = np.asarray(a)
    a00, a01, a02, a10, a11, a12, a20, a21, a22 = (a[..., k] for k in (0, 1, 2, 4, 5, 6, 8, 9, 10))
    c00, c01, c02 = a11 * a22 - a12 * a21, a12 * a20 - a10 * a22, a10 * a21 - a11 * a20
    det = (a00 * c00 + a01 * c01) + a02 * c02
    one = a.dtype.type(1.0)
    inv = one / det
    r = np.empty(a.shape, dtype=a.dtype)
    r[..., 0], r[..., 1], r[..., 2] = c00 * inv, (a02 * a21 - a01 * a22) * inv, (a01 * a12 - a02 * a11) * inv
    r[..., 4], r[..., 5], r[..., 6] = c01 * inv, (a00 * a22 - a02 * a20) * inv, (a02 * a10 - a00 * a12) * inv
    r[..., 8], r[..., 9], r[..., 10] = c02 * inv, (a01 * a20 - a00 * a21) * inv, (a00 * a11 - a01 * a10) * inv
    for i in range(3):
        r[..., 4 * i + 3] = -((r[..., 4 * i] * a[..., 3] + r[..., 4 * i + 1] * a[..., 7]) + r[..., 4 * i + 2] * a[..., 11])
    return r


def norm2(rows):
    """((w w + x x) + y y) + z z in float64 of fp32 pose rows (n, 7)."""
    w, x, y, z = (np.asarray(rows, dtype=np.float32)[..., k].astype(np.float64) for k in (3, 4, 5, 6))
    return ((w * w + x * x) + y * y) + z * z


def pose_row_to_se3(rows, fault=None, dtype=np.float64):
    """rows (n, 7) fp32 [tx ty tz qw qx qy qz] -> (n, 12)."""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 7).astype(dtype)
    w, x, y, z = (rows[:, k] for k in (3, 4, 5, 6))
    with np.errstate(all="ignore"):
        nq = ((w * w + x * x) + y * y) + z * z
        ident = nq <= IDENTITY_NORM2 if fault == "identity_le" else nq < IDENTITY_NORM2
        s = dtype(2.0) / nq
        X, Y, Z = x * s, y * s, z * s
        wX, wY, wZ, xX, xY, xZ, yY, yZ, zZ = w * X, w * Y, w * Z, x * X, x * Y, x * Z, y * Y, y * Z, z * Z
        one = dtype(1.0)
        a = np.stack([one - (yY + zZ), xY - wZ, xZ + wY, rows[:, 0], xY + wZ, one - (xX + zZ), yZ - wX, rows[:, 1],
                      xZ - wY, yZ + wX, one - (xX + yY), rows[:, 2]], axis=1)
    eye = np.tile(IDENTITY.astype(dtype), (rows.shape[0], 1))
    eye[:, [3, 7, 11]] = rows[:, :3]
    return np.where(ident[:, None], eye, a)


def to_4x4(m12):
    m12 = np.asarray(m12)
    out = np.zeros(m12.shape[:-1] + (16,), dtype=m12.dtype)
    out[..., :12] = m12
    out[..., 15] = 1.0
    return out.reshape(m12.shape[:-1] + (4, 4))


def from_4x4(m):
    return np.ascontiguousarray(np.asarray(m).reshape(m.shape[:-2] + (16,))[..., :12])


def rows_to_transforms(rows, invert=False, fault=None):
    a = pose_row_to_se3(rows, fault)
    with np.errstate(all="ignore"):
        if invert and fault != "invert_ignored":
            a = se3_inv(a)
    return to_4x4(a)


def lane_chunks(n):
    """-> (chunk, c0 (64,), c1 (64,)) of a sequence of n frames."""
    chunk = (n + 63) // 64
    c0 = np.minimum(np.arange(64) * chunk, n)
    return chunk, c0, np.minimum(c0 + chunk, n)


def _wave_scan(n, item, op, unit):
    """The scans' association: ``item(idx)`` -> the elements at rows idx, ``op(a, b)``, ``unit`` (1, k)."""
    chunk, c0, c1 = lane_chunks(n)
    val = np.repeat(unit, 64, axis=0)
    for k in range(chunk):
        on = c0 + k < c1
        val[on] = op(val[on], item(c0[on] + k))
    incl = val
    d = 1
    while d < 64:
        nxt = incl.copy()
        nxt[d:] = op(incl[:-d], incl[d:])
        incl, d = nxt, d * 2
    run = np.concatenate((unit, incl[:-1]), axis=0)
    out = np.empty((n,) + unit.shape[1:], dtype=unit.dtype)
    for k in range(chunk):
        on = c0 + k < c1
        run[on] = op(run[on], item(c0[on] + k))
        out[c0[on] + k] = run[on]
    return out


def accumulate(transforms, lengths):
    """transforms (N, 4, 4), frames of all sequences back to back -> abs (N, 4, 4), abs[f] = T[first] .. T[f]."""
    T = from_4x4(np.asarray(transforms, dtype=np.float64))
    out, lo = np.empty_like(T), 0
    for n in lengths:
        if n > 0:
            seq = T[lo:lo + n]
            out[lo:lo + n] = _wave_scan(n, lambda idx: seq[idx], se3_mul, IDENTITY[None].copy())
        lo += n
    return to_4x4(out)


def _steps(p, fault=None):
    """The length of the move INTO every frame of one sequence of positions p (n, 3): previous minus current, 0 first."""
    d = np.zeros(p.shape[0], dtype=p.dtype)
    dx, dy, dz = (p[:-1, k] - p[1:, k] for k in range(3))
    d[1:] = np.sqrt((dx * dx + dy * dy) + dz * dz)
    if fault == "first_distance_nonzero" and p.shape[0]:
        d[0] = np.sqrt((p[0, 0] * p[0, 0] + p[0, 1] * p[0, 1]) + p[0, 2] * p[0, 2])
    return d


def distances(poses, lengths, fault=None):
    """poses (N, 4, 4) -> dist (N,): dist[first] = 0, dist[f] = dist[f - 1] + |p[f - 1] - p[f]| in the scan's association."""
    p = np.asarray(poses, dtype=np.float64)[:, :3, 3]
    out, lo = np.empty(p.shape[0]), 0
    for n in lengths:
        if n > 0:
            st = _steps(p[lo:lo + n], fault)
            out[lo:lo + n] = _wave_scan(n, lambda idx: st[idx, None], lambda a, b: a + b, np.zeros((1, 1)))[:, 0]
        lo += n
    return out


def sequential_accumulate(T12, dtype):
    """The plain loop abs[f] = abs[f - 1] . T[f] on (n, 12) in ``dtype``."""
    T12 = np.asarray(T12).astype(dtype)
    out = np.empty_like(T12)
    run = IDENTITY.astype(dtype)
    for f in range(T12.shape[0]):
        run = se3_mul(run, T12[f])
        out[f] = run
    return out


def sequential_distances(p, dtype):
    st = _steps(np.asarray(p).astype(dtype))
    out, run = np.empty_like(st), dtype(0.0)
    for f in range(st.shape[0]):
        run = run + st[f]
        out[f] = run
    return out


def starts(lengths):
    return np.concatenate(([0], np.cumsum(np.asarray(lengths, dtype=np.int64)))).astype(np.int64)


def slot_counts(lengths, nlen, step):
    return [((m + step - 1) // step) * nlen for m in lengths]


def sequence_errors(gt, res, dist, lengths, segments, step, fault=None, detail=None):
    """gt, res (N, 4, 4), dist (N,) -> (err (slots, 5), valid (slots,) int32).  ``detail``: a list that receives, per valid
    slot, (slot, sequence, first, last, trace argument before the clamp, r_err, t_err)."""
    G, P = from_4x4(np.asarray(gt, dtype=np.float64)), from_4x4(np.asarray(res, dtype=np.float64))
    seq_start, nlen, nseq = starts(lengths), len(segments), len(lengths)
    slot_start = starts(slot_counts(lengths, nlen, step))
    total = int(slot_start[-1])
    err, valid = np.zeros((total, 5)), np.zeros(total, dtype=np.int32)
    for slot in range(total):
        s = 0
        while s + 1 < nseq and slot >= slot_start[s + 1]:
            s += 1
            if fault == "owner_no_empty_skip" and slot_start[s] == slot:
                break                                    # the first sequence that STARTS at this slot, empty or not
        local = slot - int(slot_start[s])
        lo, n = int(seq_start[s]), int(seq_start[s + 1] - seq_start[s])
        first, L = (local // nlen) * step, np.float64(segments[local % nlen])
        if first >= n:                                   # only a faulty owner gets here: nothing of this sequence to read
            err[slot] = [first, 0.0, 0.0, L, 0.0]
            continue
        d = dist[lo:lo + n]
        target = d[first] + L
        a, b = first, n
        while a < b:
            mid = (a + b) >> 1
            if (d[mid] >= target) if fault == "search_ge" else (d[mid] > target):
                b = mid
            else:
                a = mid + 1
        if a >= n:
            err[slot] = [first, 0.0, 0.0, L, 0.0]
            continue
        last = a - 1 if fault == "last_off_by_one" else a
        with np.errstate(all="ignore"):
            dg = se3_mul(se3_inv(G[lo + first]), G[lo + last])
            dr = se3_mul(se3_inv(P[lo + first]), P[lo + last])
            e = se3_mul(se3_inv(dr), dg)
            tr = 0.5 * (((e[0] + e[5]) + e[10]) - 1.0)
            r_err = np.arccos(tr if fault == "no_acos_clamp" else max(min(tr, 1.0), -1.0))
            t_err = np.sqrt((e[3] * e[3] + e[7] * e[7]) + e[11] * e[11])
        frames = np.float64(last - first) + 1.0
        valid[slot] = 1
        err[slot] = [first, r_err / L, t_err / L, L, L / (0.1 * frames)]
        if detail is not None:
            detail.append((slot, s, first, last, tr, r_err, t_err))
    return err, valid


def ulps(a, b):
    """Distance of float64 arrays in units in the last place (same-sign finite values and zeros; NaN -> a huge number)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ia, ib = a.view(np.int64).astype(object), b.view(np.int64).astype(object)
    fold = lambda v: np.array([int(x) if x >= 0 else -(int(x) & 0x7FFFFFFFFFFFFFFF) for x in v.reshape(-1)], dtype=object)
    d = np.abs(fold(ia) - fold(ib)).astype(np.float64)
    d[np.isnan(a.reshape(-1)) | np.isnan(b.reshape(-1))] = 2.0 ** 62
    return d.reshape(a.shape)
