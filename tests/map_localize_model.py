"""The map localiser's rule in NumPy: what ``csrc/map_localize.hip`` must reproduce.  Ranks, counts
and fp32 distances are the device's bit for bit; planes and sums are fp64.

The table of a map is an input (its slots depend on the order in which the device's insertions met): ``keys`` (T,) uint64
with EMPTY in the free slots.  ``table()`` builds one by inserting in rank order, for the tests that have no device."""
import numpy as np

import global_map_model as gm
import icp_model as icp

F = np.float32
EMPTY = np.uint64(gm.MASK)
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
LIMIT = 2 ** 31
ROW, H0, G0, SW, COST, PAIRS = icp.ROW, icp.H0, icp.G0, icp.SW, icp.COST, icp.PAIRS

FAULTS = ("tie_le", "order_swapped", "no_range_skip", "no_validation", "count_off_by_one", "max_dist_strict")


def table_slots(rows):
    L = 6
    while (1 << L) < 2 * rows:
        L += 1
    return 1 << L


def voxel_key(c):
    """c (..., 3) int64 voxel coordinates -> uint64: grid_key's hash."""
    q = np.asarray(c, dtype=np.int64).astype(np.uint64)
    with np.errstate(over="ignore"):
        return np.uint64(gm.K0) * q[..., 0] + np.uint64(gm.K1) * q[..., 1] + np.uint64(gm.K2) * q[..., 2]


def home(h, T):
    log2T = int(T).bit_length() - 1
    with np.errstate(over="ignore"):
        return int((np.uint64(h) * GOLDEN) >> np.uint64(64 - log2T))


def probe(keys, h):
    """The read-only probe -> the slot that holds h (T for the empty marker's key), -1 where an empty slot comes first."""
    T = len(keys)
    if h == EMPTY:
        return T
    slot = home(h, T)
    for _ in range(T):
        if keys[slot] == h:
            return slot
        if keys[slot] == EMPTY:
            return -1
        slot = (slot + 1) & (T - 1)
    return -1


def table(points, v, T):
    """keys (T,) of a map's points, entered in rank order."""
    keys = np.full(T, EMPTY, dtype=np.uint64)
    cand, h = gm.keys(np.asarray(points, dtype=F).reshape(-1, 3), v)
    for r in np.flatnonzero(cand):
        if h[r] == EMPTY:
            continue
        slot = home(h[r], T)
        while keys[slot] != EMPTY and keys[slot] != h[r]:
            slot = (slot + 1) & (T - 1)
        keys[slot] = h[r]
    return keys


def index(keys, points, M, v, out=None, lo=0):
    """One index pass over the ranks [lo, M) -> index (T + 1,) int32, in place where ``out`` is given."""
    T = len(keys)
    out = np.full(T + 1, -1, dtype=np.int32) if out is None else out
    if M <= lo:
        return out
    cand, h = gm.keys(np.asarray(points[:M], dtype=F).reshape(-1, 3), v)
    for r in range(max(lo, 0), M):
        if cand[r]:
            slot = probe(keys, h[r])
            if slot >= 0:
                out[slot] = r
    return out


def _slots(keys, h):
    """probe() for an array of keys: a table without deletions holds a key where the probe finds it."""
    T = len(keys)
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    pos = np.minimum(np.searchsorted(sk, h), T - 1)
    slot = np.where(sk[pos] == h, order[pos], -1)
    return np.where(h == EMPTY, T, slot)


def offsets(R, fault=None):
    w = range(-R, R + 1)
    if fault == "order_swapped":
        return np.array([(dx, dy, dz) for dx in w for dy in w for dz in w], dtype=np.int64)
    return np.array([(dx, dy, dz) for dz in w for dy in w for dx in w], dtype=np.int64)


def asked(v, q, R, fault=None):
    """q (n, 3) fp32 -> (usable (n,), h (n, N) the neighbours' keys in order, in_range (n, N): which of them are looked up)."""
    q = np.asarray(q, dtype=F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        d = q.astype(np.float64) / np.float64(v)
        inside = np.abs(d) < 2147483648.0
        c = np.rint(np.where(inside, d, 0.0)).astype(np.int64)
    nb = c[:, None, :] + offsets(R, fault)[None]
    in_range = (np.abs(nb) < LIMIT).all(axis=2)
    if fault == "no_range_skip":
        in_range = np.ones_like(in_range)
    return inside.all(axis=1), voxel_key(nb), in_range


def candidates(keys, idx, points, source, M, v, q, R, newest=None, fault=None):
    """q (n, 3) fp32 world points -> (usable (n,), rank (n, N) int64 with -1 where the neighbour yields no candidate)."""
    q = np.asarray(q, dtype=F).reshape(-1, 3)
    T = len(keys)
    usable, h, in_range = asked(v, q, R, fault)
    slot = _slots(keys, h.reshape(-1)).reshape(h.shape)
    r = np.where(slot >= 0, idx[np.maximum(slot, 0)], -1).astype(np.int64)
    ok = usable[:, None] & in_range & (slot >= 0) & (r >= 0) & (r < M)
    rr = np.where(ok, r, 0)
    pts = np.asarray(points, dtype=F).reshape(-1, 3)
    if len(pts) == 0:
        return usable, np.full(r.shape, -1, dtype=np.int64)
    cand, hk = gm.keys(pts[rr.reshape(-1)], v)
    if fault != "no_validation":
        ok &= (cand & (hk == h.reshape(-1))).reshape(h.shape)
    if newest is not None:
        ok &= np.asarray(source).reshape(-1, 2)[rr, 0] <= newest
    return usable, np.where(ok, r, -1)


def nearest(points, q, rank, fault=None):
    """-> (best rank (n,) int32, count (n,) int32, dist (n,) fp32) from the candidates' ranks in order."""
    q = np.asarray(q, dtype=F).reshape(-1, 3)
    pts = np.asarray(points, dtype=F).reshape(-1, 3)
    n, N = rank.shape
    ok = rank >= 0
    if len(pts) == 0:
        return np.full(n, -1, np.int32), np.zeros(n, np.int32), np.full(n, np.inf, F)
    m = pts[np.maximum(rank, 0)]
    with np.errstate(all="ignore"):
        e = q[:, None, :] - m
        d = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2], dtype=F)
    d = np.where(ok, d, F(np.inf))
    if fault == "tie_le":                                               # <=: the last of equal distances
        j = N - 1 - np.argmin(d[:, ::-1], axis=1)
    else:
        j = np.argmin(d, axis=1)                                        # the first of equal distances
    at = np.arange(n)
    count = ok.sum(axis=1).astype(np.int32)
    first = np.argmax(ok, axis=1) if fault != "tie_le" else N - 1 - np.argmax(ok[:, ::-1], axis=1)
    j = np.where(np.isinf(d[at, j]), first, j)                          # every distance overflowed: still a candidate's column
    best = np.where(count > 0, rank[at, j], -1).astype(np.int32)
    return best, count, np.where(count > 0, d[at, j], F(np.inf)).astype(F)


def lookup(keys, idx, points, source, M, v, q, R, newest=None, fault=None):
    _, rank = candidates(keys, idx, points, source, M, v, q, R, newest, fault)
    return nearest(points, q, rank, fault)


def planes(points, rank, best, t):
    """For every query with candidates: mean, then covariance of all candidates in order (fp64), the smallest eigenvector
    turned towards the sensor at t -> (normal (n, 3) fp64 unit or zero, eig (n, 3) ascending, gap (n,))."""
    pts = np.asarray(points, dtype=F).reshape(-1, 3).astype(np.float64)
    n = rank.shape[0]
    ok = rank >= 0
    k = ok.sum(axis=1)
    m = pts[np.maximum(rank, 0)] * ok[..., None]
    with np.errstate(all="ignore"):
        mu = np.cumsum(m, axis=1)[:, -1] / k[:, None]
        d = np.where(ok[..., None], pts[np.maximum(rank, 0)] - mu[:, None, :], 0.0)
        cov = np.cumsum(d[..., :, None] * d[..., None, :], axis=1)[:, -1]
    cov = np.where(np.isfinite(cov), cov, 0.0)
    val, vec = np.linalg.eigh(cov)
    nrm = vec[:, :, 0].copy()
    y = pts[np.maximum(best, 0)]
    flip = np.einsum("ni,ni->n", nrm, y - np.asarray(t, dtype=np.float64)[None]) > 0.0
    nrm[flip] *= -1.0
    bad = ~(val[:, 1] > icp.RANK_EPS * val[:, 2]) | (k < 1)
    nrm[bad] = 0.0
    with np.errstate(all="ignore"):
        gap = np.where(val[:, 2] > 0.0, (val[:, 1] - val[:, 0]) / val[:, 2], 0.0)
    return nrm, val, gap


def accumulate(keys, idx, points, source, M, v, p, T, R, sigma, max_dist, min_neighbours=5, newest=None, normals=None,
               fault=None):
    """One stream -> (sum (32,), sum of |term| (32,), dict(rank, count, dist, normal, pair)).  T (4, 4) or None (p are world
    points, the sensor at the origin).  ``normals`` (n, 3) fp32: use these instead of the model's own planes."""
    p = np.asarray(p, dtype=F).reshape(-1, 3)
    Tm = np.eye(4) if T is None else np.asarray(T, dtype=np.float64)
    q = p if T is None else gm.world(p, Tm)
    usable, rank = candidates(keys, idx, points, source, M, v, q, R, newest, fault)
    best, count, dist = nearest(points, q, rank, fault)
    need = min_neighbours + 1 if fault == "count_off_by_one" else min_neighbours
    with np.errstate(invalid="ignore"):
        near = (dist < F(max_dist)) if fault == "max_dist_strict" else (dist <= F(max_dist))
    fit = usable & (best >= 0) & (count >= need) & near
    nrm = np.zeros((len(p), 3))
    if normals is not None:
        nrm[fit] = np.asarray(normals, dtype=F)[fit].astype(np.float64)
    elif fit.any():
        nrm[fit] = planes(points, rank[fit], best[fit], Tm[:3, 3])[0]
    n32 = nrm.astype(F)
    pair = fit & (n32 != 0).any(axis=1)
    out, mag = np.zeros((ROW,)), np.zeros((ROW,))
    near_out = dict(rank=best, count=count, dist=dist, normal=n32, pair=pair)
    sel = np.flatnonzero(pair)
    if sel.size == 0:
        return out, mag, near_out
    pts = np.asarray(points, dtype=F).reshape(-1, 3)
    y, nn, qq = pts[best[sel]].astype(np.float64), n32[sel].astype(np.float64), q[sel].astype(np.float64)
    r = (nn[:, 0] * (qq[:, 0] - y[:, 0]) + nn[:, 1] * (qq[:, 1] - y[:, 1])) + nn[:, 2] * (qq[:, 2] - y[:, 2])
    pp = p[sel].astype(np.float64) @ Tm[:3, :3].T + Tm[:3, 3]
    J = np.concatenate([np.cross(pp, nn), nn], axis=1)
    w2 = icp.huber_w2(r, sigma)
    for e, (a, b) in enumerate(icp.UPPER):
        t = w2 * J[:, a] * J[:, b]
        out[H0 + e], mag[H0 + e] = t.sum(), np.abs(t).sum()
    for a in range(6):
        t = w2 * J[:, a] * r
        out[G0 + a], mag[G0 + a] = t.sum(), np.abs(t).sum()
    out[SW] = mag[SW] = w2.sum()
    out[COST] = mag[COST] = (w2 * r * r).sum()
    out[PAIRS] = mag[PAIRS] = float(sel.size)
    return out, mag, near_out


def localize(keys, idx, points, source, M, v, cloud, init, R=1, iters=10, sigma=0.5, max_dist=None, min_neighbours=5,
             damping=1e-6, threshold=1e-4, min_pairs=64, newest=None):
    """The whole localisation of one stream -> (T, status, list of per-iteration dicts)."""
    max_dist = largest_max_dist(R, v) if max_dist is None else max_dist
    T, status, steps = np.array(init, dtype=np.float64), 0, []
    for it in range(iters):
        row, _, near = accumulate(keys, idx, points, source, M, v, cloud, T, R, sigma, max_dist, min_neighbours, newest)
        s = icp.solve(row, T, status, it, damping, threshold, min_pairs)
        T, status = s["T"], s["status"]
        steps.append(dict(row=row, delta=s["delta"], T=T, status=status, pairs=int(row[PAIRS])))
    return T, status, steps


def largest_max_dist(R, v):
    bound = float(R) * float(v)
    f = F(bound)
    if float(f) > bound:
        f = np.nextafter(f, F(0.0))
    return float(f)


def brute_nearest(points, q):
    """fp32 distance of every query to its nearest map point, over the whole map -> (dist (n,), rank (n,))."""
    q, pts = np.asarray(q, dtype=F).reshape(-1, 3), np.asarray(points, dtype=F).reshape(-1, 3)
    e = q[:, None, :] - pts[None]
    d = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2], dtype=F)
    j = np.argmin(d, axis=1)
    return d[np.arange(len(q)), j], j


class Map:
    """One stream's map on the host with a table and an index of its own: what the CPU tests localise in."""

    def __init__(self, clouds, X, v, frames=None, capacity=None, T=None):
        self.v = v
        self.points, self.source, total = gm.build(clouds, X, v, frames=frames, capacity=capacity)
        self.M = len(self.points)
        self.T = T or table_slots(int(np.prod(np.asarray(clouds).shape[:2])))
        self.keys = table(self.points, v, self.T)
        self.index = index(self.keys, self.points, self.M, v)

    def args(self):
        return self.keys, self.index, self.points, self.source, self.M, self.v
