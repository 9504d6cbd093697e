"""NumPy host model of ``batches.TrainBatchBuilder`` (a test helper: not a conftest, not a product module).

Written from the rules of DESIGN.md section 13, not from the kernels:

* Philox4x32-10, key = (seed low word, seed high word), counter = (index, unit, step mod 2^32, purpose), purposes
  0 = selection keys (unit = cloud 2 * pair + frame, index = row), 1 = draws with replacement (unit = cloud, index = draw
  number), 2 = augmentation (unit = pair, index = 0..5 = parameter number).  Output word 0 is "the word"; a normal uses
  words 0 and 1.
* Selection: ``count >= npoints``: the ``npoints`` survivors with the smallest ``(word << 32) | row``, ascending;
  ``0 < count < npoints``: all survivors in frame order, then draw j = survivor number ``(word_j * count) >> 32``;
  ``count == 0``: row ``(word_j * n) >> 32`` for j = 0 .. npoints-1.
* Normal: ``sqrt(-2 ln u1) cos(2 pi u2)``, ``u = (word + 0.5) * 2^-32``; parameter = fp32(clip(scale * z)).
* ``n == 0`` rows (only reachable with device lengths, which the kernel clamps to ``[0, R]``): every point has index -1 and
  coordinates +0.0, count 0.  ``build(..., clamp_lengths=True)`` applies the clamp.
* Pose algebra as the reference's datasets do it (see the builder's docstring).

``select_rows_stable`` states the subset rule a second time without the 64-bit key; ``select_info`` and ``wave_layout`` read
off what a case reaches (threshold word, ``ties``, ``need``; the kernel's row ranges per wave).  ``fault=`` plants one of
``FAULTS`` for tests/test_train_batch_cases_cpu.py: each is a way the kernel could be wrong, never used by a GPU test.
"""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
SELECT, REPLACE, AUGMENT = 0, 1, 2
AUG_SCALE = np.array([0.01, 0.05, 0.01, 0.1, 0.05, 0.5])
AUG_CLIP = np.array([0.02, 0.1, 0.02, 0.2, 0.15, 1.0])
KITTI360_GROUND_Z = -(1.73 - 0.3)
MASK = np.uint64(0xFFFFFFFF)
FAULTS = ("tie_high_row", "tie_all", "tie_none", "count_gt", "no_clamp", "n0_row0", "quat_ge", "no_gimbal", "sort_pow2")


def philox4x32_10(counter, key):
    """counter: 4 broadcastable uint32-valued arrays, key: 2 -> 4 uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k0, p1 & MASK, (p0 >> s32) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return [v.astype(np.uint32) for v in c]


def words(index, unit, step, purpose, seed, n_out=1):
    seed = int(seed) & ((1 << 64) - 1)
    out = philox4x32_10((index, unit, int(step) & 0xFFFFFFFF, purpose), (seed & 0xFFFFFFFF, seed >> 32))
    return out[0] if n_out == 1 else out[:n_out]


def select_info(keep, npoints, cloud, step, seed):
    """What the radix select ends with for ``count >= npoints``: the threshold word (the ``npoints``-th smallest among the
    survivors'), ``smaller`` survivors below it, ``ties`` at it, ``need = npoints - smaller`` of them to take."""
    surv = np.nonzero(keep)[0]
    w = np.sort(words(surv, cloud, step, SELECT, seed))
    t = w[npoints - 1]
    smaller, ties = int((w < t).sum()), int((w == t).sum())
    return dict(threshold=int(t), smaller=smaller, ties=ties, need=npoints - smaller)


def select_rows_stable(keep, npoints, cloud, step, seed):
    """The subset rule once more, without packing keys: survivors ordered by (word, row), the first ``npoints``."""
    surv = np.nonzero(keep)[0]
    w = words(surv, cloud, step, SELECT, seed)
    return surv[np.lexsort((surv, w))[:npoints]].astype(np.int64)


def wave_layout(n):
    """(per_wave, [(i0, i1)] * 16): the contiguous row range of each of the 16 waves."""
    per_wave = ((n + 15) // 16 + 63) // 64 * 64
    return per_wave, [(w * per_wave, min(n, w * per_wave + per_wave)) for w in range(16)]


def _faulty_subset(surv, w, npoints, fault):
    """The subset a kernel with ``fault`` would give: what is collected (in frame order, as far as the ``npoints`` real
    slots go), then sorted by key."""
    t = np.sort(w)[npoints - 1]
    need = npoints - int((w < t).sum())
    tied = np.nonzero(w == t)[0]
    take = w < t
    if fault == "tie_high_row":
        take[tied[len(tied) - need:]] = True
    elif fault == "tie_all":
        take[tied] = True
    elif fault != "tie_none":
        take[tied[:need]] = True
    got = np.nonzero(take)[0][:npoints]
    keys = (w[got].astype(np.uint64) << np.uint64(32)) | surv[got].astype(np.uint64)
    keys = np.concatenate([keys, np.full(npoints - len(got), ~np.uint64(0))])       # a slot nothing was written to
    if fault == "sort_pow2":
        p2 = 1 << (npoints.bit_length() - 1)
        return np.concatenate([np.sort(keys[:p2]), keys[p2:]])
    return np.sort(keys)


def select_rows(keep, npoints, cloud, step, seed, fault=None):
    """keep: (n,) bool mask over the rows both frames share -> (rows (npoints,) int64, count)."""
    n = keep.shape[0]
    if n == 0:
        return np.full(npoints, 0 if fault == "n0_row0" else -1, dtype=np.int64), 0
    surv = np.nonzero(keep)[0]
    count = len(surv)
    if count > npoints or (count == npoints and fault != "count_gt"):
        w = words(surv, cloud, step, SELECT, seed)
        if fault in ("tie_high_row", "tie_all", "tie_none", "sort_pow2"):
            keys = _faulty_subset(surv, w, int(npoints), fault)
        else:
            keys = np.sort((w.astype(np.uint64) << np.uint64(32)) | surv.astype(np.uint64))[:npoints]
        return (keys & MASK).astype(np.uint32).view(np.int32).astype(np.int64), count
    j = np.arange(npoints - count)
    w = words(j, cloud, step, REPLACE, seed).astype(np.uint64)
    if count > 0:
        return np.concatenate([surv, surv[((w * np.uint64(count)) >> np.uint64(32)).astype(np.int64)]]), count
    return ((w * np.uint64(n)) >> np.uint64(32)).astype(np.int64), 0


def draw_aug(pair, step, seed):
    """-> (6,) float32 (anglex, angley, anglez, xx, yy, zz), clipped, angles before ``* pi / 4``."""
    w0, w1 = words(np.arange(6), pair, step, AUGMENT, seed, n_out=2)
    u1 = (w0.astype(np.float64) + 0.5) * 2.0 ** -32
    u2 = (w1.astype(np.float64) + 0.5) * 2.0 ** -32
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    return np.clip(AUG_SCALE * z, -AUG_CLIP, AUG_CLIP).astype(np.float32)


def t_trans_of(params):
    """(6,) float32 -> (4,4) float64: [Rx . Ry . Rz | (xx, yy, zz)]."""
    ax, ay, az = (np.float64(params[i]) * np.pi / 4.0 for i in range(3))
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rx.dot(Ry).dot(Rz)
    T[:3, 3] = np.asarray(params[3:6], dtype=np.float64)
    return T


def inv_rigid(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return out


def quat_zyx(R, fault=None):
    """Rotation matrix -> (w, x, y, z) through the zyx Euler angles (the KITTI dataset's mat2euler + euler2quat)."""
    r11, r12, r13, r21, r22, r23, _r31, _r32, r33 = np.asarray(R, dtype=np.float64).flat
    cy = np.sqrt(r33 * r33 + r23 * r23)
    if cy > np.finfo(np.float64).eps * 4 or fault == "no_gimbal":
        z, y, x = np.arctan2(-r12, r11), np.arctan2(r13, cy), np.arctan2(-r23, r33)
    else:
        z, y, x = np.arctan2(r21, r22), np.arctan2(r13, cy), 0.0
    z, y, x = z / 2.0, y / 2.0, x / 2.0
    cz, sz, cy, sy, cx, sx = np.cos(z), np.sin(z), np.cos(y), np.sin(y), np.cos(x), np.sin(x)
    return np.array([cx * cy * cz - sx * sy * sz, cx * sy * sz + cy * cz * sx, cx * cz * sy - sx * cy * sz,
                     cx * cy * sz + sx * cz * sy])


def quat_branch(R, fault=None):
    """0, 1, 2 = m00, m11, m22, 3 = trace: the FIRST largest of the four (np.argmax; the kernel's strict ``>`` walk)."""
    R = np.asarray(R, dtype=np.float64)
    dec = [R[0, 0], R[1, 1], R[2, 2], (R[0, 0] + R[1, 1]) + R[2, 2]]
    return 3 - int(np.argmax(dec[::-1])) if fault == "quat_ge" else int(np.argmax(dec))


def quat_diag(R, fault=None):
    """Rotation matrix -> (w, x, y, z): the largest of (m00, m11, m22, trace) picks the form, then normalise."""
    R = np.asarray(R, dtype=np.float64)
    tr = (R[0, 0] + R[1, 1]) + R[2, 2]
    ch = quat_branch(R, fault)
    v = np.empty(4)
    if ch != 3:
        i = ch
        j = (i + 1) % 3
        k = (j + 1) % 3
        v[i] = 1.0 - tr + 2.0 * R[i, i]
        v[j] = R[j, i] + R[i, j]
        v[k] = R[k, i] + R[i, k]
        v[3] = R[k, j] - R[j, k]
    else:
        v[0] = R[2, 1] - R[1, 2]
        v[1] = R[0, 2] - R[2, 0]
        v[2] = R[1, 0] - R[0, 1]
        v[3] = 1.0 + tr
    v = v / np.sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3])
    return np.array([v[3], v[0], v[1], v[2]])


def pose(dataset, t_diff, params, fault=None):
    """t_diff (4,4) / (3,4) f64, params (6,) f32 or None (no augmentation) -> (T_trans, T_gt (4,4) f64, gt (7,) f32)."""
    Td = np.eye(4)
    Td[:3] = np.asarray(t_diff, dtype=np.float64)[:3]
    if params is None:
        Tt, Tg = np.eye(4), Td
    else:
        Tt = t_trans_of(params)
        Tg = Td @ inv_rigid(Tt) if dataset == "kitti" else Tt @ Td
    q = quat_zyx(Tg[:3, :3], fault) if dataset == "kitti" else quat_diag(Tg[:3, :3], fault)
    return Tt, Tg, np.concatenate([Tg[:3, 3], q]).astype(np.float32)


def filter_rows(dataset, rows, tr=None, near=30.0, ground_z=KITTI360_GROUND_Z):
    """rows (n,4) f32 -> (xyz (n,3) f32, keep (n,) bool): the arithmetic of csrc/rows.hpp (fp64 transform summed left to
    right and stored as fp32 for KITTI; fp32 comparisons for KITTI-360)."""
    if dataset == "kitti":
        t = np.asarray(tr, dtype=np.float64)[:3]
        x, y, z = (rows[:, i].astype(np.float64) for i in range(3))
        o = np.stack([((t[r, 0] * x + t[r, 1] * y) + t[r, 2] * z) + t[r, 3] for r in range(3)], axis=1)
        keep = ~(o[:, 1] > 1.1) & (o[:, 0] < 30.0) & (o[:, 0] > -30.0) & (o[:, 2] < 30.0) & (o[:, 2] > -30.0)
        return o.astype(np.float32), keep
    g, nr = np.float32(ground_z), np.float32(near)
    keep = ~(rows[:, 2] < g) & (rows[:, 0] < nr) & (rows[:, 0] > -nr) & (rows[:, 1] < nr) & (rows[:, 1] > -nr)
    return rows[:, :3].copy(), keep


def apply_trans(T, xyz):
    """T (4,4) f64, xyz (m,3) f32 -> (m,3) f32: fp64, summed left to right, rounded once."""
    x, y, z = (xyz[:, i].astype(np.float64) for i in range(3))
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1).astype(np.float32)


def build(dataset, sweeps, lengths, t_diff, npoints, seed, step, augment=True, aug=None, tr=None, near=30.0,
          ground_z=KITTI360_GROUND_Z, clamp_lengths=False, fault=None):
    """The whole batch: sweeps (B,2,R,4) f32, lengths (B,2), t_diff (B,4|3,4) f64, tr (3,4) or (B,3,4) -> dict of
    xyz_f1, xyz_f2 (B,3,npoints) f32, gt (B,7) f32, indices (2B,npoints) i32, counts (2B,) i32, aug (B,6) f32,
    t_gt (B,4,4) f64, t_trans (B,4,4) f64.  ``clamp_lengths``: the lengths are a device tensor's, which the kernel clamps
    to [0, R] (host lengths are refused outside [1, R] before any launch)."""
    B, R = sweeps.shape[0], sweeps.shape[2]
    out = dict(xyz_f1=np.zeros((B, 3, npoints), np.float32), xyz_f2=np.zeros((B, 3, npoints), np.float32),
               gt=np.zeros((B, 7), np.float32), indices=np.zeros((2 * B, npoints), np.int32),
               counts=np.zeros((2 * B,), np.int32), aug=np.zeros((B, 6), np.float32), t_gt=np.zeros((B, 4, 4)),
               t_trans=np.zeros((B, 4, 4)))
    if tr is not None:
        tr = np.asarray(tr, dtype=np.float64)
        tr = np.broadcast_to(tr[None] if tr.ndim == 2 else tr, (B,) + tr.shape[-2:])
    for b in range(B):
        if clamp_lengths and fault != "no_clamp":
            n = int(min(min(max(int(lengths[b][0]), 0), R), min(max(int(lengths[b][1]), 0), R)))
        else:
            n = max(int(min(lengths[b][0], lengths[b][1])), 0)
        params = None
        if augment:
            params = np.asarray(aug[b], dtype=np.float32) if aug is not None else draw_aug(b, step, seed)
            out["aug"][b] = params
        Tt, Tg, gt = pose(dataset, t_diff[b], params, fault)
        out["t_trans"][b], out["t_gt"][b], out["gt"][b] = Tt, Tg, gt
        clouds = []
        for f in range(2):
            xyz, keep = filter_rows(dataset, sweeps[b, f, :n], None if tr is None else tr[b], near, ground_z)
            if fault == "no_clamp" and n > R:                 # rows past the frame: whatever lies there; no row survives
                xyz, keep = np.concatenate([xyz, np.zeros((n - R, 3), np.float32)]), np.concatenate([keep, np.zeros(n - R, bool)])
            rows, count = select_rows(keep, npoints, 2 * b + f, step, seed, fault)
            out["indices"][2 * b + f], out["counts"][2 * b + f] = rows, count
            pts = xyz[rows] if n > 0 else np.zeros((npoints, 3), np.float32)
            if n == 0 and fault == "n0_row0":
                pts = np.tile(filter_rows(dataset, sweeps[b, f, :1], None if tr is None else tr[b], near, ground_z)[0], (npoints, 1))
            if f == 1 and augment and (n > 0 or fault == "n0_row0"):      # a zero point of an empty frame is not moved
                pts = apply_trans(Tt, pts)
            clouds.append(pts.T)
        first, second = (clouds[1], clouds[0]) if dataset == "kitti" else (clouds[0], clouds[1])
        out["xyz_f1"][b], out["xyz_f2"][b] = first, second
    return out
