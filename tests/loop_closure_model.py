"""NumPy model of the loop detector: the specification restated, not the kernels' code.

Nothing could be recorded from the reference (its detector needs cv2), so this model is what the GPU tests pin.  The fp32
functions evaluate every expression in the order the specification fixes, with NumPy float32 scalars and arrays, so the
kernels (built without contraction) must repeat them bit for bit; the ``*64`` functions are the plain fp64 restatement the
fp32 model is itself checked against."""
import numpy as np

F = np.float32


def tables(rings, sectors, max_range):
    k = np.arange(1, rings + 1, dtype=np.float64)
    ring_b = ((k * float(max_range) / rings) ** 2).astype(F)
    ang = 2.0 * np.pi * np.arange(sectors, dtype=np.float64) / sectors
    return ring_b, np.cos(ang).astype(F), np.sin(ang).astype(F)


def permute(cloud, up):
    """The descriptor's (x, y, z) of the rows: as they are, or (z_cam, -x_cam, -y_cam) for KITTI's camera frame."""
    c = np.asarray(cloud, dtype=F)
    return (c[:, 0], c[:, 1], c[:, 2]) if up == "z" else (c[:, 2], -c[:, 0], -c[:, 1])


def bins(cloud, rings=20, sectors=60, max_range=80.0, z_offset=2.0, up="z", length=None):
    """-> (keep (n,) bool, ring (n,), sector (n,), h (n,) fp32).  Every sector is evaluated; a kept point must lie in exactly
    one (asserted: the specification promises it for sectors >= 8)."""
    x, y, z = permute(cloud, up)
    n = len(x)
    ring_b, dx, dy = tables(rings, sectors, max_range)
    with np.errstate(all="ignore"):
        r2 = x * x + y * y
        h = z + F(z_offset)
        finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        keep = finite & ~(r2 >= ring_b[-1]) & ~(r2 == 0) & (h > 0)
        if length is not None:
            keep &= np.arange(n) < max(0, min(int(length), n))
        ring = (ring_b[None, :rings - 1] <= r2[:, None]).sum(axis=1)
        cross = dx[None, :] * y[:, None] - dy[None, :] * x[:, None]
        dot = dx[None, :] * x[:, None] + dy[None, :] * y[:, None]
        inside = (dot > 0) & (cross >= 0) & (np.roll(cross, -1, axis=1) < 0)
    assert np.all(inside[keep].sum(axis=1) == 1), "a kept point lies in no sector or in two"
    return keep, ring, inside.argmax(axis=1), h


def descriptor(cloud, rings=20, sectors=60, max_range=80.0, z_offset=2.0, up="z", length=None):
    """-> (D (NR, NS) fp32, Dn, mask as a Python int)."""
    keep, ring, sector, h = bins(cloud, rings, sectors, max_range, z_offset, up, length)
    D = np.zeros((rings, sectors), dtype=F)
    np.maximum.at(D, (ring[keep], sector[keep]), h[keep])
    return (D,) + normalise(D)


def normalise(D):
    rings, sectors = D.shape
    total = np.zeros(sectors, dtype=F)
    for r in range(rings):
        total = total + D[r] * D[r]
    norm = np.sqrt(total)
    with np.errstate(all="ignore"):
        Dn = np.where(norm > 0, D / norm[None, :], F(0)).astype(F)
    mask = 0
    for j in range(sectors):
        if norm[j] > 0:
            mask |= 1 << j
    return Dn, mask


def rotate(mask, sectors, s):
    full = (1 << sectors) - 1
    return ((mask >> s) | (mask << (sectors - s))) & full


def distances(Qn, qmask, En, emask):
    """Q (NR, NS), E (ne, NR, NS), emask list of ints -> d (ne, NS) fp32: j outer, r inner, unfused."""
    rings, sectors = Qn.shape
    En = np.asarray(En, dtype=F).reshape(-1, rings, sectors)
    Q2 = np.concatenate([Qn, Qn], axis=1)
    shifts = np.arange(sectors)
    c = np.zeros((len(En), sectors), dtype=F)
    for j in range(sectors):
        for r in range(rings):
            c = c + Q2[r, j + shifts][None, :] * En[:, r, j][:, None]
    v = np.array([[bin(rotate(qmask, sectors, s) & int(m)).count("1") for s in range(sectors)] for m in emask], dtype=F)
    v = v.reshape(len(En), sectors)
    with np.errstate(all="ignore"):
        return np.where(v > 0, F(1) - c / v, F(np.inf)).astype(F)


def distances64(Qn, qmask, En, emask):
    rings, sectors = Qn.shape
    En = np.asarray(En, dtype=np.float64).reshape(-1, rings, sectors)
    Q = np.asarray(Qn, dtype=np.float64)
    d = np.full((len(En), sectors), np.inf)
    for s in range(sectors):
        c = np.einsum("rj,erj->e", np.roll(Q, -s, axis=1), En)
        for e, m in enumerate(emask):
            v = bin(rotate(qmask, sectors, s) & int(m)).count("1")
            if v:
                d[e, s] = 1.0 - c[e] / v
    return d


def descriptor64(cloud, rings=20, sectors=60, max_range=80.0, z_offset=2.0, up="z"):
    """The plain restatement: polar bins from fp64 radius and angle."""
    c = np.asarray(cloud, dtype=np.float64)
    x, y, z = (c[:, 0], c[:, 1], c[:, 2]) if up == "z" else (c[:, 2], -c[:, 0], -c[:, 1])
    r, h = np.hypot(x, y), z + z_offset
    keep = np.isfinite(c).all(axis=1) & (r < max_range) & (r > 0) & (h > 0)
    ring = np.minimum((r / (max_range / rings)).astype(np.int64), rings - 1)
    sector = (np.floor(np.mod(np.arctan2(y, x), 2 * np.pi) / (2 * np.pi / sectors)).astype(np.int64)) % sectors
    D = np.zeros((rings, sectors))
    np.maximum.at(D, (ring[keep], sector[keep]), h[keep])
    norm = np.sqrt((D * D).sum(axis=0))
    Dn = np.divide(D, norm[None, :], out=np.zeros_like(D), where=norm[None, :] > 0)
    return D, Dn, sum(1 << j for j in range(sectors) if norm[j] > 0)


def eligible(frame_ids, f, min_id_distance, positions=None, max_distance=None):
    """positions: (frames, 3) fp64 read by frame id; the gate compares squared distances, (dx dx + dy dy) + dz dz."""
    frame_ids = np.asarray(frame_ids, dtype=np.int64)
    ok = frame_ids + min_id_distance <= f
    if positions is not None and max_distance is not None:
        p = np.asarray(positions, dtype=np.float64)
        inside = (frame_ids >= 0) & (frame_ids < len(p)) & (0 <= f < len(p))
        d = p[np.clip(frame_ids, 0, len(p) - 1)] - p[min(max(f, 0), len(p) - 1)]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        ok &= inside & (d2 < max_distance * max_distance)
    return ok


def search(Qn, qmask, En, emask, frame_ids, f, min_id_distance, threshold, positions=None, max_distance=None, dist=distances):
    """-> dict(scores (ne,), shifts (ne,), found, entry, frame_i, shift, score): ineligible entries score +inf with shift 0;
    the lowest score wins, the lowest entry on a tie; a match where the score is below the threshold."""
    ne = len(emask)
    scores, shifts = np.full(ne, np.inf, dtype=F if dist is distances else np.float64), np.zeros(ne, dtype=np.int64)
    if ne:
        ok = eligible(frame_ids, f, min_id_distance, positions, max_distance)
        if ok.any():
            d = dist(Qn, qmask, np.asarray(En)[ok], [m for m, o in zip(emask, ok) if o])
            scores[ok], shifts[ok] = d.min(axis=1), d.argmin(axis=1)         # argmin: the first (smallest) shift
    out = dict(scores=scores, shifts=shifts, found=0, entry=-1, frame_i=-1, shift=0, score=np.inf)
    if ne and np.isfinite(scores.min()):
        e = int(scores.argmin())
        out.update(entry=e, frame_i=int(frame_ids[e]), shift=int(shifts[e]), score=scores[e],
                   found=int(scores[e] < (F(threshold) if dist is distances else threshold)))
    return out


def start_pose(shift, sectors, up="z"):
    """T0: the pose of the query in the stored frame, Rz(-shift 2 pi / NS), conjugated for ``up="-y"``."""
    a = -shift * 2.0 * np.pi / sectors
    Rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    P = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]]) if up == "-y" else np.eye(3)
    T = np.eye(4)
    T[:3, :3] = P.T @ Rz @ P
    return T
