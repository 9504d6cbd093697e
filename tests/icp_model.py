"""NumPy fp64 model of the point-to-plane registration of csrc/icp.hpp / icp.hip, and the scenes
its tests use.  It restates the reference's local_map.py (normals) and optimization.py (Huber weights, Gauss-Newton) by
reading them; the reference itself is not run.  Neighbour choices use the fp32 key of include/pwclo_ops.h,
sqrtf(((dx*dx + dy*dy) + dz*dz) + 1e-8f), so that they are the device's bit for bit; everything else is fp64."""
import numpy as np

ROW = 32
H0, G0, SW, COST, PAIRS = 0, 21, 27, 28, 29
CONVERGED, FEW_PAIRS, BAD_PIVOT = 1, 2, 4
RANK_EPS = 1e-10
HUBER_CLAMP = 1e-4
EPS64 = np.finfo(np.float64).eps
UPPER = [(i, j) for i in range(6) for j in range(i, 6)]


# ---- neighbours ------------------------------------------------------------------------------------------------------------

def key32(queries, cloud):
    """(s, 3), (n, 3) fp32 -> (s, n) fp32 keys, every operation rounded to binary32 in the header's order."""
    q, c = np.asarray(queries, dtype=np.float32), np.asarray(cloud, dtype=np.float32)
    d = q[:, None, :] - c[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return np.sqrt(d2 + np.float32(1e-8), dtype=np.float32)


def knn(queries, cloud, k):
    """The k nearest of every query, ascending key, equal keys by ascending index -> (idx (s, k) int32, key (s, k) fp32)."""
    key = key32(queries, cloud)
    if k == 1:                                                   # argmin returns the first (lowest) index of the minimum
        idx = np.argmin(key, axis=1)[:, None]
        return idx.astype(np.int32), np.take_along_axis(key, idx, axis=1)
    idx = np.argsort(key, axis=1, kind="stable")[:, :k]
    return idx.astype(np.int32), np.take_along_axis(key, idx, axis=1)


# ---- normals ---------------------------------------------------------------------------------------------------------------

def normals(xyz, k):
    """xyz (n, 3) fp32 -> (normal (n, 3) fp64 unit or zero, eig (n, 3) ascending, gap (n,) = (l_mid - l_min) / l_max)."""
    xyz = np.asarray(xyz, dtype=np.float32)
    idx, _ = knn(xyz, xyz, k + 1)
    x = xyz.astype(np.float64)
    d = x[idx[:, 1:]] - x[:, None, :]
    cov = np.einsum("nki,nkj->nij", d, d)
    val, vec = np.linalg.eigh(cov)
    nrm = vec[:, :, 0].copy()
    flip = np.einsum("ni,ni->n", nrm, x) > 0.0
    nrm[flip] *= -1.0
    bad = ~(val[:, 1] > RANK_EPS * val[:, 2])
    nrm[bad] = 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = np.where(val[:, 2] > 0.0, (val[:, 1] - val[:, 0]) / val[:, 2], 0.0)
    return nrm, val, gap


def eig3(c):
    """icp_eig3 restated operation for operation (8 sweeps of cyclic Jacobi over (0,1), (0,2), (1,2)): c = [xx xy xz yy yz zz]
    -> (val (3,) ascending, vec (3,) the unit eigenvector of val[0]).  Where np.linalg.eigh leaves a sign or a basis of a
    repeated eigenvalue open, this is the device's choice."""
    a = np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]], dtype=np.float64)
    v = np.eye(3)
    with np.errstate(all="ignore"):
        for _ in range(8):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                apq = a[p, q]
                if apq == 0.0 or apq != apq:
                    continue
                theta = (a[q, q] - a[p, p]) / (2.0 * apq)
                t = (-1.0 if theta < 0.0 else 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                cs = 1.0 / np.sqrt(t * t + 1.0)
                sn = t * cs
                o = 3 - p - q
                app, aqq, aop, aoq = a[p, p], a[q, q], a[o, p], a[o, q]
                a[p, p], a[q, q] = app - t * apq, aqq + t * apq
                a[p, q] = a[q, p] = 0.0
                a[o, p] = a[p, o] = cs * aop - sn * aoq
                a[o, q] = a[q, o] = sn * aop + cs * aoq
                for i in range(3):
                    vip, viq = v[i, p], v[i, q]
                    v[i, p], v[i, q] = cs * vip - sn * viq, sn * vip + cs * viq
        d0, d1, d2 = a[0, 0], a[1, 1], a[2, 2]
        lo = 0 if (d0 <= d1 and d0 <= d2) else (1 if d1 <= d2 else 2)
        e1, e2 = (d1 if lo == 0 else d0), (d1 if lo == 2 else d2)
        val = np.array([(d0, d1, d2)[lo], e1 if e1 <= e2 else e2, e2 if e1 <= e2 else e1])
        x, y, z = v[0, lo], v[1, lo], v[2, lo]
        inv = 1.0 / np.sqrt((x * x + y * y) + z * z)
        return val, np.array([x * inv, y * inv, z * inv])


# ---- queries, accumulate, solve, push --------------------------------------------------------------------------------------

def queries(A, p, T=None):
    """A (M, 4, 4), p (n, 3) fp32, T (4, 4) -> (q fp64 (M, n, 3) before rounding, its fp32 rounding)."""
    p64 = np.asarray(p, dtype=np.float32).astype(np.float64)
    out = []
    for m in range(A.shape[0]):
        a = A[m] if T is None else A[m] @ T
        out.append(p64 @ a[:3, :3].T + a[:3, 3])
    q = np.stack(out)
    return q, q.astype(np.float32)


def search(q32, map_xyz):
    """q32 (M, n, 3), map_xyz (M, n, 3) -> (idx (M, n) int32, dist (M, n) fp32): the search with nsample = 1 per slot."""
    idx, dist = [], []
    for m in range(q32.shape[0]):
        i, d = knn(q32[m], map_xyz[m], 1)
        idx.append(i[:, 0])
        dist.append(d[:, 0])
    return np.stack(idx), np.stack(dist)


def huber_w2(r, sigma):
    ar = np.abs(r)
    cl = np.maximum(ar, HUBER_CLAMP)
    return np.where(ar < sigma, 1.0, (2.0 * sigma * ar - sigma * sigma) / (cl * cl))


def choose(dist, live, max_dist):
    """dist (M, n) fp32, live (M,) -> (slot (n,) of the smallest dist among the live slots, lower slot on a tie; ok (n,))."""
    M, n = dist.shape
    best, bd = np.full((n,), -1), np.zeros((n,), dtype=np.float32)
    for m in range(M):
        if not live[m]:
            continue
        with np.errstate(invalid="ignore"):
            take = (best < 0) | (dist[m] < bd)
        best = np.where(take, m, best)
        bd = np.where(take, dist[m], bd)
    with np.errstate(invalid="ignore"):
        ok = (best >= 0) & (bd <= np.float32(max_dist))
    return best, ok


def accumulate(p, q32, idx, dist, map_xyz, map_normals, live, R, T, sigma, max_dist, points=None):
    """One stream.  -> (sum (32,), sum of |term| (32,)) over the pairs; the inputs as the device kernel takes them.
    ``points``: a slice of point indices; only their pairs are added (one workgroup's row: tests/icp_cases.py)."""
    n = p.shape[0]
    slot, ok = choose(dist, live, max_dist)
    if points is not None:
        inside = np.zeros((n,), dtype=bool)
        inside[points] = True
        ok = ok & inside
    sel = np.flatnonzero(ok)
    out, mag = np.zeros((ROW,)), np.zeros((ROW,))
    if sel.size == 0:
        return out, mag
    m = slot[sel]
    j = idx[m, sel]
    inb = (j >= 0) & (j < n)
    sel, m, j = sel[inb], m[inb], j[inb]
    y = map_xyz[m, j].astype(np.float64)
    nn = map_normals[m, j].astype(np.float64)
    keep = (map_normals[m, j] != 0).any(axis=1)
    sel, m, y, nn = sel[keep], m[keep], y[keep], nn[keep]
    q = q32[m, sel].astype(np.float64)
    r = np.einsum("ni,ni->n", nn, q - y)
    npr = np.einsum("nij,nj->ni", R[m], nn)
    pp = p[sel].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    J = np.concatenate([np.cross(pp, npr), npr], axis=1)
    w2 = huber_w2(r, sigma)
    for e, (a, b) in enumerate(UPPER):
        t = w2 * J[:, a] * J[:, b]
        out[H0 + e], mag[H0 + e] = t.sum(), np.abs(t).sum()
    for a in range(6):
        t = w2 * J[:, a] * r
        out[G0 + a], mag[G0 + a] = t.sum(), np.abs(t).sum()
    out[SW] = mag[SW] = w2.sum()
    out[COST] = mag[COST] = (w2 * r * r).sum()
    out[PAIRS] = mag[PAIRS] = float(sel.size)
    return out, mag


def system(row, damping):
    """A row of sums -> (H / sw + damping I (6, 6), g / sw (6,))."""
    H = np.zeros((6, 6))
    for e, (a, b) in enumerate(UPPER):
        H[a, b] = H[b, a] = row[H0 + e] / row[SW]
    return H + damping * np.eye(6), row[G0:G0 + 6] / row[SW]


def exp_update(delta, T):
    """[Rodrigues(w) | v] T with the rotation re-orthonormalised by Gram-Schmidt on its columns, as icp_update_pose."""
    w, v = delta[:3], delta[3:]
    th = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    a, b = 1.0, 0.5
    if th > 0.0:
        a = np.sin(th) / th
        h = np.sin(0.5 * th) / (0.5 * th)
        b = 0.5 * h * h
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    E = np.eye(4)
    E[:3, :3] = np.eye(3) + a * K + b * (K @ K)
    E[:3, 3] = v
    N = E @ T
    c0 = N[:3, 0] / np.linalg.norm(N[:3, 0])
    c1 = N[:3, 1] - (c0 @ N[:3, 1]) * c0
    c1 = c1 / np.linalg.norm(c1)
    out = np.eye(4)
    out[:3, 0], out[:3, 1], out[:3, 2], out[:3, 3] = c0, c1, np.cross(c0, c1), N[:3, 3]
    return out


def solve(row, T, status, it, damping, threshold, min_pairs):
    """One stream, one solver launch -> dict(delta, T, status, moved: whether iterations / pairs / cost were recorded)."""
    if it == 0:
        status = 0
    delta = np.zeros((6,))
    if status != 0:
        return dict(delta=delta, T=T.copy(), status=status, moved=False)
    if int(row[PAIRS]) < min_pairs:
        return dict(delta=delta, T=T.copy(), status=FEW_PAIRS, moved=True)
    H, g = system(row, damping)
    try:
        with np.errstate(all="ignore"):
            L = np.linalg.cholesky(H)
        if not np.isfinite(L).all():
            raise np.linalg.LinAlgError
    except np.linalg.LinAlgError:
        return dict(delta=delta, T=T.copy(), status=BAD_PIVOT, moved=True)
    z = np.linalg.solve(L, g)
    delta = -np.linalg.solve(L.T, z)
    if not np.isfinite(delta).all():                            # a NaN in g alone passes every pivot: icp_solve6 refuses the step
        return dict(delta=np.zeros((6,)), T=T.copy(), status=BAD_PIVOT, moved=True)
    new = exp_update(delta, T)
    return dict(delta=delta, T=new, status=CONVERGED if np.linalg.norm(delta) < threshold else 0, moved=True)


class Map:
    """One stream's map: slots of (cloud fp32, normals fp32), A (M, 4, 4), R (M, 3, 3), live (M,), cursor."""

    def __init__(self, M, n, k):
        self.M, self.n, self.k = M, n, k
        self.xyz = np.zeros((M, n, 3), dtype=np.float32)
        self.normals = np.zeros((M, n, 3), dtype=np.float32)
        self.reset()

    def reset(self):
        self.A = np.tile(np.eye(4), (self.M, 1, 1))
        self.R = np.tile(np.eye(3), (self.M, 1, 1))
        self.live = np.zeros((self.M,), dtype=np.int32)
        self.cursor = 0

    def push(self, cloud, T, normals32=None):
        slot = self.cursor
        for m in range(self.M):
            if m != slot and self.live[m]:
                self.A[m] = self.A[m] @ T
                self.R[m] = T[:3, :3].T @ self.R[m]
        self.A[slot], self.R[slot], self.live[slot] = np.eye(4), np.eye(3), 1
        self.xyz[slot] = cloud
        self.normals[slot] = normals(cloud, self.k)[0].astype(np.float32) if normals32 is None else normals32
        self.cursor = (slot + 1) % self.M


def register(mp, cloud, init, iters=10, sigma=0.5, max_dist=1.0, damping=1e-6, threshold=1e-4, min_pairs=64, push=True):
    """The whole registration of one stream's frame against ``mp`` -> (T, status, list of per-iteration dicts)."""
    T, status, steps = np.array(init, dtype=np.float64), 0, []
    cloud = np.asarray(cloud, dtype=np.float32)
    for it in range(iters):
        _, q32 = queries(mp.A, cloud, T)
        idx, dist = search(q32, mp.xyz)
        row, _ = accumulate(cloud, q32, idx, dist, mp.xyz, mp.normals, mp.live, mp.R, T, sigma, max_dist)
        s = solve(row, T, status, it, damping, threshold, min_pairs)
        T, status = s["T"], s["status"]
        steps.append(dict(row=row, delta=s["delta"], T=T, status=status))
    if push:
        mp.push(cloud, T)
    return T, status, steps


# ---- poses and scenes ------------------------------------------------------------------------------------------------------

def rot(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def pose_error(T, gt):
    """|translation difference| in metres + the angle of the rotation difference in radians."""
    d = np.linalg.inv(gt) @ T
    c = np.clip((np.trace(d[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.linalg.norm(T[:3, 3] - gt[:3, 3]) + np.arccos(c))


ROOM = np.array([3.0, 2.5, 1.5])              # half extents: walls x = +-3, y = +-2.5, floor and ceiling z = +-1.5


def room(seed, frames, n, noise=0.01, walls_only=False):
    """A box room seen from a sensor that moves 0.1-0.2 m and turns up to 2 degrees (about a tilted axis) per frame; every
    frame samples its own n ray directions and gets its own range noise.  Six planes, three mutually non-parallel pairs;
    ``walls_only`` keeps the four walls (two directions), so that translation along z is unobservable.
    -> (clouds (frames, n, 3) fp32 in the sensor frames, T (frames, 4, 4): T[k] maps frame k into frame k - 1, T[0] = I)."""
    r = np.random.default_rng([seed, frames, n, int(walls_only)])
    world = [np.eye(4)]
    for _ in range(frames - 1):
        axis = np.array([0.0, 0.0, 1.0]) if walls_only else np.array([0.3, -0.2, 1.0])
        step = pose(rot(axis, np.deg2rad(r.uniform(-2.0, 2.0))),
                    np.array([r.uniform(0.1, 0.2), r.uniform(-0.05, 0.05), 0.0 if walls_only else r.uniform(-0.03, 0.03)]))
        world.append(world[-1] @ step)
    clouds = np.empty((frames, n, 3), dtype=np.float32)
    for k, W in enumerate(world):
        pts = np.empty((0, 3))
        while pts.shape[0] < n:
            d = r.normal(size=(2 * n, 3))
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            if walls_only:
                d = d[np.abs(d[:, 2]) < 0.3]
            dw = d @ W[:3, :3].T
            with np.errstate(divide="ignore"):
                t = np.where(dw > 0, (ROOM - W[:3, 3]) / dw, (-ROOM - W[:3, 3]) / dw)      # exit distance per axis
            face = np.argmin(t, axis=1)
            rng = t[np.arange(len(d)), face]
            keep = np.isfinite(rng) & ((face < 2) if walls_only else True)
            rng = rng + r.normal(0.0, noise, len(d))
            pts = np.concatenate([pts, (d * rng[:, None])[keep]])
        clouds[k] = pts[:n]
    T = np.stack([np.eye(4)] + [np.linalg.inv(world[k - 1]) @ world[k] for k in range(1, frames)])
    return clouds, T


def perturbed(T, deg=2.0, shift=0.3):
    """T off by ``deg`` degrees about a fixed tilted axis and ``shift`` metres along a fixed direction."""
    d = np.array([0.6, -0.64, 0.48])
    return pose(rot([0.2, 0.5, 1.0], np.deg2rad(deg)), shift * d) @ T


# ---- inputs shared by the CPU and the GPU tests ----------------------------------------------------------------------------

NORMAL_SHAPES = [(b, n, k) for n in (64, 65, 1000, 1024) for k in (3, 10, 63) for b in (1, 3)]
GAP_MIN, GAP_CAP = 1e-3, 0.02               # points below the relative eigen-gap are left out, at most 2 % of a cloud


def normals_cloud(b, n, seed=5):
    """b clouds of n points in a 4 m cube around (1, 2, 8): a third on each of two noisy planes, the rest in the volume."""
    r = np.random.default_rng([seed, b, n])
    out = np.empty((b, n, 3), dtype=np.float32)
    for c in range(b):
        p = r.uniform(-2.0, 2.0, (n, 3))
        third = n // 3
        p[:third, 2] = 0.3 * p[:third, 0] + r.normal(0.0, 0.02, third)
        p[third:2 * third, 0] = -0.5 * p[third:2 * third, 1] + 1.0 + r.normal(0.0, 0.02, third)
        out[c] = (p + np.array([1.0, 2.0, 8.0])).astype(np.float32)
    return out


def planted(seed=11, S=3, M=3, n=300, sigma=0.5, max_dist=1.0):
    """Inputs of one accumulate launch with every case of its contract: ties between slots (stream 0: slots 0 / 1, stream
    1: slots 0 / 2 around a dead slot 1 that holds NaNs and wild indices), dist == max_dist exactly, |r| on both sides of
    sigma, zero normals, n no multiple of 64 and more than one workgroup, and a stream (2) whose points are all rejected."""
    r = np.random.default_rng([seed, S, M, n])
    p = r.uniform(-5.0, 5.0, (S, n, 3)).astype(np.float32)
    T = np.stack([pose(rot(r.normal(size=3), 0.05), r.normal(size=3) * 0.1) for _ in range(S)])
    A = np.stack([np.stack([pose(rot(r.normal(size=3), r.uniform(0, 0.3)), r.normal(size=3)) for _ in range(M)])
                  for _ in range(S)])
    R = np.ascontiguousarray(np.transpose(A[:, :, :3, :3], (0, 1, 3, 2)))
    q = np.stack([queries(A[s], p[s], T[s])[1] for s in range(S)])
    idx = r.integers(0, n, (S, M, n)).astype(np.int32)
    dist = r.uniform(0.0, 1.4 * max_dist, (S, M, n)).astype(np.float32)
    map_normals = r.normal(size=(S, M, n, 3))
    map_normals = (map_normals / np.linalg.norm(map_normals, axis=-1, keepdims=True)).astype(np.float32)
    map_normals[:, :, ::17] = 0.0
    map_xyz = np.zeros((S, M, n, 3), dtype=np.float32)
    scale = np.where(r.random((S, M, n, 1)) < 0.5, 0.1, 2.0)
    for s in range(S):
        for m in range(M):
            map_xyz[s, m, idx[s, m]] = q[s, m] + (scale[s, m] * r.normal(size=(n, 3))).astype(np.float32)
    live = np.ones((S, M), dtype=np.int32)
    dist[0, 1, ::5] = dist[0, 0, ::5]                                   # ties: the lower slot must win
    dist[0, 2, ::5] = np.float32(2.0 * max_dist)
    live[1, 1] = 0                                                      # a dead slot: nothing of it may be read
    dist[1, 1], map_xyz[1, 1], map_normals[1, 1], idx[1, 1] = np.nan, np.nan, np.nan, 1 << 30
    dist[1, 2, ::3] = dist[1, 0, ::3]
    dist[1, 0, 1::7] = np.float32(max_dist)                             # exactly the bound: kept
    dist[1, 2, 1::7] = np.float32(max_dist)
    if S > 2:
        dist[2] = np.nextafter(np.float32(max_dist), np.float32(np.inf))      # one ulp above: every point rejected
    return dict(p=p, q=q, idx=idx, dist=dist, map_xyz=map_xyz, map_normals=map_normals, live=live, R=R, T=T, sigma=sigma,
                max_dist=max_dist)


def planted_rows(seed=23, n=400, flat=False, pairs=None):
    """A row of sums from well-spread synthetic pairs; ``flat``: every normal has z = 0 and R = I, so that the row and
    column of translation along z are exactly zero (the walls-only case); ``pairs``: use only that many points."""
    r = np.random.default_rng([seed, n, int(flat)])
    n = n if pairs is None else pairs
    p = r.uniform(-5.0, 5.0, (n, 3)).astype(np.float32)
    nn = r.normal(size=(n, 3))
    if flat:
        nn[:, 2] = 0.0
    nn = (nn / np.linalg.norm(nn, axis=1, keepdims=True)).astype(np.float32)
    y = (p + r.normal(0.0, 0.2, (n, 3))).astype(np.float32)
    one = lambda a: a[None]
    row, _ = accumulate(p, one(p), one(np.arange(n, dtype=np.int32)), np.zeros((1, n), dtype=np.float32), one(y), one(nn),
                        np.ones((1,), dtype=np.int32), one(np.eye(3)), np.eye(4), 0.5, 1.0)
    return row
