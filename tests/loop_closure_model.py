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
    with np.errstate(all="ignore"):                      # a square may overflow: the norm is inf then, the column 0
        for r in range(rings):
            total = total + D[r] * D[r]
        norm = np.sqrt(total)
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


# ---- the bookkeeping stages: select, accept, insert, fetch and the words of build ---------------------------------------------

FEW_PAIRS, BAD_PIVOT = 2, 4                             # the refiner's status bits that refuse a closure
NO_MATCH = (0, -1, -1, 0)


def build_words(active, restart, count, nlog, epoch):
    """The detector's words after build: an idle stream keeps all three; ``restart`` empties an active one."""
    if active != 0 and restart != 0:
        return 0, 0, epoch + 1
    return count, nlog, epoch


def build(cloud, length, active, restart, count, nlog, epoch, **params):
    """-> None for an idle stream (nothing is written), else dict(D, Dn, mask, count, nlog, epoch)."""
    if active == 0:
        return None
    D, Dn, mask = descriptor(cloud, length=length, **params)
    count, nlog, epoch = build_words(active, restart, count, nlog, epoch)
    return dict(D=D, Dn=Dn, mask=mask, count=count, nlog=nlog, epoch=epoch)


def select(scores, shifts, frame_ids, count, active, f, stride, threshold, MK):
    """-> dict(match (found, entry, frame_i, shift), score fp32, found, slot, overflow, row): the lowest score below +inf
    wins (a NaN never does), the lowest entry on a tie (-0.0 == 0.0 is one); ``row``: the row of the T0 table, None for the
    identity.  The slot: ``count`` where the stream is active, f >= 0, f % stride == 0 and count < MK; a full database
    raises overflow; an idle stream gets the no-match record and slot -1."""
    out = dict(match=NO_MATCH, score=F(np.inf), found=0, slot=-1, overflow=False, row=None)
    if not active:
        return out
    v = np.asarray(scores, dtype=F)[:MK]
    wins = v < F(np.inf)                                 # false for NaN and for +inf
    if wins.any():
        e = int(np.nonzero(wins & (v == v[wins].min()))[0][0])
        d = v[e]                                         # the winner's own bits: -0.0 and 0.0 compare equal
        found = int(d < F(threshold))
        out.update(match=(found, e, int(frame_ids[e]), int(shifts[e])), score=d, found=found,
                   row=int(shifts[e]) if found else None)
    if f >= 0 and f % stride == 0:
        if count < MK:
            out["slot"] = int(count)
        else:
            out["overflow"] = True
    return out


def accept(found, match, score, f, T, status, pairs, cost, n, min_fitness, max_mean_cost, nlog, ML):
    """-> dict(accepted, nlog, overflow, record): refused where a status bit 2 or 4 is set, not ``pairs >= min_fitness n``
    or not ``cost / pairs <= max_mean_cost`` (fp64, so a NaN on either side refuses); ``status=None``: every match, with
    pairs 0 and cost 0.  record: None or (log_i (4,) int32, log_T (4, 4) fp64, log_c (2,) fp64); a full log raises overflow."""
    out = dict(accepted=0, nlog=int(nlog), overflow=False, record=None)
    if not found:
        return out
    if status is None:
        pairs, cost = 0, np.float64(0.0)
    else:
        pairs, cost = int(pairs), np.float64(cost)
        if status & (FEW_PAIRS | BAD_PIVOT):
            return out
        with np.errstate(all="ignore"):
            if not (np.float64(pairs) >= np.float64(min_fitness) * np.float64(n)):
                return out
            if not (cost / np.float64(pairs) <= np.float64(max_mean_cost)):
                return out
    if nlog >= ML:
        out["overflow"] = True
        return out
    rec = (np.array([match[2], f, match[3], pairs], dtype=np.int32), np.array(T, dtype=np.float64).reshape(4, 4),
           np.array([np.float64(F(score)), cost], dtype=np.float64))
    out.update(accepted=1, nlog=int(nlog) + 1, record=rec)
    return out


def insert(slot, f, Qn, qmask, cloud, MK):
    """-> None (nothing is written) or dict(entry, desc (NS, NR): the columns of Qn, each contiguous, mask, frame, cloud,
    count = slot + 1 whatever the count held)."""
    if slot < 0 or slot >= MK:
        return None
    return dict(entry=int(slot), desc=np.ascontiguousarray(np.asarray(Qn, dtype=F).T), mask=int(qmask), frame=int(f),
                cloud=None if cloud is None else np.asarray(cloud, dtype=F), count=int(slot) + 1)


def fetch(found, match, db_cloud, MK):
    """-> None (staging keeps its words) or the matched entry's (n, 3) cloud."""
    e = match[1]
    if not found or e < 0 or e >= MK:
        return None
    return np.asarray(db_cloud, dtype=F)[e]
