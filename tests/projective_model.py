"""NumPy model of the projective frame-to-model registration of csrc/projective.hpp / projective.hip (DESIGN.md section
22): projection, z-buffer, normal map, model build, association and the registration loop, with the sums and the solve
taken from tests/icp_model.py.  A point's pixel is computed in fp32 in the device's (the reference's) order of operations;
``margin`` says in fp64 how far the coordinates are from a rounding boundary or a validity limit, so that a test can keep
its inputs away from where the last bit of an fp32 atan2 / asin decides.  Everything else is fp64.

``planted(name)`` makes the model wrong in one named way (FAULTS) for as long as the block lasts: tests/test_projective_cases_cpu.py
uses it to prove that a case of tests/projective_cases.py tells the right answer from the wrong one."""
import contextlib

import numpy as np

import icp_model as icp

EMPTY = -1
DET_EPS = np.float32(1e-6)
F = np.float32
TILE_H, TILE_W = 8, 32                           # csrc/projective.hip: PROJ_TILE_H, PROJ_TILE_W

FAULTS = {
    "seam_wrap": "a column that rounds to W wraps to column 0 instead of being refused",
    "half_up": "rows and columns round half up, not half to even",
    "tie_highest": "a z-buffer keeps the highest index among equal ranges",
    "ignore_range": "a z-buffer keeps the lowest index, whatever the ranges",
    "halo_low": "a tile of the normal map stages one pixel less of border above and to the left",
    "halo_high": "a tile of the normal map stages one pixel less of border below and to the right",
    "edge_next_row": "the normal map's bounds check lets column W through, which is the next row's column 0",
    "slot_tie_le": "association takes a later slot at an equal distance (<= for <)",
    "max_dist_lt": "association refuses a pair at exactly max_dist (< for <=)",
    "zero_normal_skip": "association skips a slot without a normal instead of refusing the pair",
    "no_cursor_clamp": "the handover uses the cursor as it is: a slot of a neighbouring stream, or nothing",
}
FAULT = None


@contextlib.contextmanager
def planted(name):
    global FAULT
    assert name in FAULTS and FAULT is None
    FAULT = name
    try:
        yield
    finally:
        FAULT = None


def image(H, W, up_fov, down_fov):
    up, down = up_fov / 180.0 * np.pi, down_fov / 180.0 * np.pi
    return dict(H=int(H), W=int(W), down=F(abs(down)), fov=F(abs(down) + abs(up)), down64=abs(down),
                fov64=abs(down) + abs(up))


def pixels(pts, im):
    """pts (n, >=3) fp32 -> (row, col int64 (n,), r fp32 (n,), valid (n,), margin (n,) fp64 px).  ``margin``: the smallest
    distance of the fp64 row / column from a rounding boundary (x.5), which also bounds the distance from the validity
    limits -0.5 and H - 0.5 / W - 0.5; inf for points without a range."""
    p = np.asarray(pts, dtype=np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    H, W = im["H"], im["W"]
    with np.errstate(all="ignore"):
        r = np.sqrt((x * x + y * y) + z * z, dtype=np.float32)
        theta = -np.arctan2(y, x, dtype=np.float32)
        phi = np.arcsin(z / r, dtype=np.float32)
        col = (F(0.5) * (theta / F(np.pi) + F(1.0))) * F(W)
        row = (F(1.0) - (phi + im["down"]) / im["fov"]) * F(H)
        rr, rc = np.rint(row), np.rint(col)
        if FAULT == "half_up":
            rr, rc = np.floor(row + F(0.5)), np.floor(col + F(0.5))
        if FAULT == "seam_wrap":
            rc = np.where(rc == W, F(0.0), rc)
        valid = (r > 0) & np.isfinite(r) & (rr >= 0) & (rr <= H - 1) & (rc >= 0) & (rc <= W - 1)
        p64 = p.astype(np.float64)
        r64 = np.sqrt((p64[:, :3] ** 2).sum(axis=1))
        col64 = 0.5 * (-np.arctan2(p64[:, 1], p64[:, 0]) / np.pi + 1.0) * W
        row64 = (1.0 - (np.arcsin(p64[:, 2] / r64) + im["down64"]) / im["fov64"]) * H
        frac = lambda v: np.abs(np.abs(v - np.floor(v)) - 0.5)
        margin = np.where((r64 > 0) & np.isfinite(r64), np.minimum(frac(row64), frac(col64)), np.inf)
    margin = np.where(np.isnan(margin), np.inf, margin)
    ri = np.where(valid, rr, 0).astype(np.int64)
    ci = np.where(valid, rc, 0).astype(np.int64)
    return ri, ci, r, valid, margin


def coords(pts, im):
    """pts (n, >=3) fp32 -> dict(row32, col32: the fp32 coordinates before rounding, as ``pixels`` computes them; row64, col64:
    the same in fp64; r: the fp32 range).  For tests that have to know where a point lies, not only which pixel it gets."""
    p = np.asarray(pts, dtype=np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    H, W = im["H"], im["W"]
    with np.errstate(all="ignore"):
        r = np.sqrt((x * x + y * y) + z * z, dtype=np.float32)
        col = (F(0.5) * (-np.arctan2(y, x, dtype=np.float32) / F(np.pi) + F(1.0))) * F(W)
        row = (F(1.0) - (np.arcsin(z / r, dtype=np.float32) + im["down"]) / im["fov"]) * F(H)
        p64 = p.astype(np.float64)
        r64 = np.sqrt((p64[:, :3] ** 2).sum(axis=1))
        col64 = 0.5 * (-np.arctan2(p64[:, 1], p64[:, 0]) / np.pi + 1.0) * W
        row64 = (1.0 - (np.arcsin(p64[:, 2] / r64) + im["down64"]) / im["fov64"]) * H
    return dict(row32=row, col32=col, row64=row64, col64=col64, r=r)


def zbuffer(pix, r, valid, HW):
    """pix (n,) pixel indices, r (n,) fp32 ranges -> winner (HW,) int64: per pixel the index of the smallest r, the lowest
    index among equal r; -1 for an empty pixel."""
    win = np.full((HW,), EMPTY, dtype=np.int64)
    idx = np.flatnonzero(valid)
    if idx.size:
        tie = -idx if FAULT == "tie_highest" else idx
        rng = np.zeros_like(r[idx]) if FAULT == "ignore_range" else r[idx]
        order = idx[np.lexsort((tie, rng, pix[idx]))]             # by pixel, then range, then index
        first = np.ones(order.size, dtype=bool)
        first[1:] = pix[order][1:] != pix[order][:-1]
        win[pix[order][first]] = order[first]
    return win


def vertex_map(points, im, length=None, keep=None):
    """points (R, 3|4) fp32 -> (vmap (H, W, 3) fp32, rows (H, W) int32): one stream."""
    p = np.asarray(points, dtype=np.float32)
    R = p.shape[0]
    row, col, r, valid, _ = pixels(p, im)
    if length is not None:
        valid = valid & (np.arange(R) < min(max(int(length), 0), R))
    if keep is not None:
        valid = valid & (np.asarray(keep) != 0)
    H, W = im["H"], im["W"]
    win = zbuffer(row * W + col, r, valid, H * W)
    vmap = np.zeros((H * W, 3), dtype=np.float32)
    vmap[win >= 0] = p[win[win >= 0], :3]
    return vmap.reshape(H, W, 3), win.astype(np.int32).reshape(H, W)


def moments(vmap, k):
    """vmap (H, W, 3) fp32 -> (m (H, W, 3), C (H, W, 3, 3)) fp64 over the k x k window with zero padding."""
    H, W, _ = vmap.shape
    h = k // 2
    v = np.zeros((H + 2 * h, W + 2 * h, 3))
    v[h:h + H, h:h + W] = vmap.astype(np.float64)
    if FAULT == "edge_next_row":
        v[h:h + H - 1, h + W] = vmap[1:, 0].astype(np.float64)
    lo, hi = h - (FAULT == "halo_low"), h - (FAULT == "halo_high")
    ys, xs = np.arange(H), np.arange(W)
    y0, x0 = ys // TILE_H * TILE_H, xs // TILE_W * TILE_W
    m, C = np.zeros((H, W, 3)), np.zeros((H, W, 3, 3))
    for dy in range(k):
        for dx in range(k):
            w = v[dy:dy + H, dx:dx + W]
            if lo < h or hi < h:                                   # what the pixel's own tile did not stage reads as zero
                sy, sx = ys + dy - h, xs + dx - h
                w = w.copy()
                w[(sy < y0 - lo) | (sy >= y0 + TILE_H + hi)] = 0.0
                w[:, (sx < x0 - lo) | (sx >= x0 + TILE_W + hi)] = 0.0
            m += w
            C += w[..., :, None] * w[..., None, :]
    return m, C


def normal_map(vmap, k=5):
    """compute_normal_map in fp64 -> (n (H, W, 3) fp64 unit or zero, det (H, W) fp64)."""
    vmap = np.asarray(vmap, dtype=np.float32)
    m, C = moments(vmap, k)
    det = np.linalg.det(C)
    ok = np.abs(det.astype(np.float32)) > DET_EPS
    n = np.zeros_like(m)
    if ok.any():
        n[ok] = np.linalg.solve(C[ok], m[ok][..., None])[..., 0]
    ln = np.linalg.norm(n, axis=-1)
    ok &= (ln > 0) & np.isfinite(ln) & (vmap != 0).any(axis=-1)
    n = np.where(ok[..., None], n / np.where(ln > 0, ln, 1.0)[..., None], 0.0)
    return n, det


def inverse(A):
    out = np.eye(4)
    out[:3, :3] = A[:3, :3].T
    out[:3, 3] = -A[:3, :3].T @ A[:3, 3]
    return out


def model_build(map_v, map_n, A, live, im):
    """map_v / map_n (M, H, W, 3) fp32, A (M, 4, 4): the newest frame -> slot, live (M,) -> dict(v, n (M, H, W, 3): the
    fp64 products before rounding, src (M, H, W) int32, margin (M, H * W): of every moved source pixel, inf where empty)."""
    M, H, W, _ = map_v.shape
    HW = H * W
    v, n = np.zeros((M, HW, 3)), np.zeros((M, HW, 3))
    src = np.full((M, HW), EMPTY, dtype=np.int32)
    margin = np.full((M, HW), np.inf)
    for m in range(M):
        if not live[m]:
            continue
        inv = inverse(A[m])
        p = map_v[m].reshape(HW, 3)
        occupied = (p != 0).any(axis=1)
        moved = p.astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]
        rot = map_n[m].reshape(HW, 3).astype(np.float64) @ inv[:3, :3].T
        row, col, r, valid, mg = pixels(moved.astype(np.float32), im)
        margin[m] = np.where(occupied, mg, np.inf)
        win = zbuffer(row * W + col, r, valid & occupied, HW)
        has = win >= 0
        v[m, has], n[m, has], src[m, has] = moved[win[has]], rot[win[has]], win[has]
    return dict(v=v.reshape(M, H, W, 3), n=n.reshape(M, H, W, 3), src=src.reshape(M, H, W), margin=margin)


def associate(vmap, model_v, model_n, T, im, max_dist, pixel=None):
    """One stream: vmap (H, W, 3) fp32, model_v / model_n (M, H, W, 3) fp32, T (4, 4) -> dict(q32 (HW, 3), pixel (HW,)
    (-1: source empty or no pixel), slot (HW,) (-1: no pair), margin (HW,), gap (HW,): relative distance gap between the best
    and the second-best slot, inf with fewer than two candidates).  ``pixel``: use these pixels instead of the model's own."""
    H, W = im["H"], im["W"]
    HW, M = H * W, model_v.shape[0]
    p = np.asarray(vmap, dtype=np.float32).reshape(HW, 3)
    q32 = (p.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    occupied = (p != 0).any(axis=1)
    row, col, _, valid, margin = pixels(q32, im)
    own = np.where(valid & occupied, row * W + col, EMPTY)
    pix = own if pixel is None else np.asarray(pixel, dtype=np.int64)
    mv, mn = model_v.reshape(M, HW, 3), model_n.reshape(M, HW, 3)
    at = np.clip(pix, 0, HW - 1)
    best, bd = np.full((HW,), EMPTY), np.zeros((HW,), dtype=np.float32)
    second = np.full((HW,), np.inf)
    for m in range(M):
        y = mv[m, at]
        d = q32 - y
        dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], dtype=np.float32)
        cand = (pix >= 0) & (y != 0).any(axis=1)
        if FAULT == "zero_normal_skip":
            cand &= (mn[m, at] != 0).any(axis=1)
        with np.errstate(invalid="ignore"):
            take = cand & ((best < 0) | ((dist <= bd) if FAULT == "slot_tie_le" else (dist < bd)))
        second = np.where(take & (best >= 0), bd, np.where(cand & ~take, np.minimum(second, dist), second))
        best = np.where(take, m, best)
        bd = np.where(take, dist, bd)
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.where(np.isfinite(second), (second - bd) / np.maximum(second, 1e-30), np.inf)
        ok = (best >= 0) & ((bd < np.float32(max_dist)) if FAULT == "max_dist_lt" else (bd <= np.float32(max_dist)))
    ok &= (mn[np.clip(best, 0, M - 1), at] != 0).any(axis=1)
    return dict(q32=q32, pixel=pix, own_pixel=own, slot=np.where(ok, best, EMPTY), margin=np.where(occupied, margin, np.inf),
                gap=gap, dist=bd)


def accumulate(vmap, model_v, model_n, T, im, sigma, max_dist, pixel=None):
    """One stream -> (sum (32,), sum of |term| (32,), the association): icp_model's row over the projective pairs."""
    a = associate(vmap, model_v, model_n, T, im, max_dist, pixel)
    H, W = im["H"], im["W"]
    HW, M = H * W, model_v.shape[0]
    sel = np.flatnonzero(a["slot"] >= 0)
    out, mag = np.zeros((icp.ROW,)), np.zeros((icp.ROW,))
    if sel.size == 0:
        return out, mag, a
    m, at = a["slot"][sel], a["pixel"][sel]
    y = model_v.reshape(M, HW, 3)[m, at].astype(np.float64)
    nn = model_n.reshape(M, HW, 3)[m, at].astype(np.float64)
    p = np.asarray(vmap, dtype=np.float32).reshape(HW, 3)[sel].astype(np.float64)
    q = a["q32"][sel].astype(np.float64)
    r = np.einsum("ni,ni->n", nn, q - y)
    pp = p @ T[:3, :3].T + T[:3, 3]
    J = np.concatenate([np.cross(pp, nn), nn], axis=1)
    w2 = icp.huber_w2(r, sigma)
    for e, (i, j) in enumerate(icp.UPPER):
        t = w2 * J[:, i] * J[:, j]
        out[icp.H0 + e], mag[icp.H0 + e] = t.sum(), np.abs(t).sum()
    for i in range(6):
        t = w2 * J[:, i] * r
        out[icp.G0 + i], mag[icp.G0 + i] = t.sum(), np.abs(t).sum()
    out[icp.SW] = mag[icp.SW] = w2.sum()
    out[icp.COST] = mag[icp.COST] = (w2 * r * r).sum()
    out[icp.PAIRS] = mag[icp.PAIRS] = float(sel.size)
    return out, mag, a


class Map:
    """One stream's map: slots of (vertex map, normal map) fp32, A (M, 4, 4): the newest frame -> slot, live, cursor."""

    def __init__(self, M, H, W):
        self.M = M
        self.v = np.zeros((M, H, W, 3), dtype=np.float32)
        self.n = np.zeros((M, H, W, 3), dtype=np.float32)
        self.reset()

    def reset(self):
        self.A = np.tile(np.eye(4), (self.M, 1, 1))
        self.live = np.zeros((self.M,), dtype=np.int32)
        self.cursor = 0

    def push(self, vmap, nmap, T):
        slot = self.cursor
        for m in range(self.M):
            if m != slot and self.live[m]:
                self.A[m] = self.A[m] @ T
        self.A[slot], self.live[slot] = np.eye(4), 1
        self.v[slot], self.n[slot] = vmap, nmap
        self.cursor = (slot + 1) % self.M


def map_push(T, vmap, nmap, map_v, map_n, A, live, cursor):
    """The handover of every stream, in place, as projective.map_push: T (S, 4, 4), vmap / nmap (S, H, W, 3), map_v / map_n
    (S, M, H, W, 3), A (S, M, 4, 4), live (S, M), cursor (S,).  A cursor outside [0, M) is clamped first."""
    S, M = live.shape
    fv, fn = map_v.reshape((S * M,) + map_v.shape[2:]), map_n.reshape((S * M,) + map_n.shape[2:])
    for s in range(S):
        slot = min(max(int(cursor[s]), 0), M - 1)
        if FAULT == "no_cursor_clamp":
            slot = int(cursor[s])
        if 0 <= s * M + slot < S * M:
            fv[s * M + slot], fn[s * M + slot] = vmap[s], nmap[s]
        for m in range(M):
            if m == slot:
                A[s, m], live[s, m] = np.eye(4), 1
            elif live[s, m]:
                A[s, m] = A[s, m] @ T[s]
        cursor[s] = 0 if slot + 1 == M else slot + 1


def register(mp, vmap, nmap, init, im, iters=10, sigma=0.5, max_dist=1.0, damping=1e-6, threshold=1e-4, min_pairs=64,
             push=True):
    """The whole registration of one stream's frame (its vertex and normal map, fp32) -> (T, status, steps)."""
    built = model_build(mp.v, mp.n, mp.A, mp.live, im)
    mv, mn = built["v"].astype(np.float32), built["n"].astype(np.float32)
    T, status, steps = np.array(init, dtype=np.float64), 0, []
    for it in range(iters):
        row, _, _ = accumulate(vmap, mv, mn, T, im, sigma, max_dist)
        s = icp.solve(row, T, status, it, damping, threshold, min_pairs)
        T, status = s["T"], s["status"]
        steps.append(dict(row=row, delta=s["delta"], T=T, status=status))
    if push:
        mp.push(vmap, nmap, T)
    return T, status, steps


# ---- scenes ------------------------------------------------------------------------------------------------------------------

def beams(im, jitter=None):
    """Unit directions through the pixel centres of the image (H * W, 3), optionally jittered by ``jitter`` (H * W, 2) px."""
    H, W = im["H"], im["W"]
    row, col = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    row, col = row.reshape(-1), col.reshape(-1)
    if jitter is not None:
        row, col = row + jitter[:, 0], col + jitter[:, 1]
    phi = (1.0 - row / H) * im["fov64"] - im["down64"]
    theta = (2.0 * col / W - 1.0) * np.pi
    return np.stack([np.cos(phi) * np.cos(-theta), np.cos(phi) * np.sin(-theta), np.sin(phi)], axis=1)


def room_scans(seed, frames, im, noise=0.01, band=1e-3):
    """icp_model's box room scanned along the image's beams (jittered by up to 0.3 px, own range noise per frame) by a
    sensor that moves as ``icp_model.room``'s does.  Points whose fp64 pixel lies within ``band`` px of a rounding boundary
    are left out (their rows become the origin, which has no pixel).  -> (clouds (frames, H * W, 3) fp32, T (frames, 4, 4))."""
    r = np.random.default_rng([seed, frames, im["H"], im["W"]])
    world = [np.eye(4)]
    for _ in range(frames - 1):
        step = icp.pose(icp.rot(np.array([0.3, -0.2, 1.0]), np.deg2rad(r.uniform(-2.0, 2.0))),
                        np.array([r.uniform(0.1, 0.2), r.uniform(-0.05, 0.05), r.uniform(-0.03, 0.03)]))
        world.append(world[-1] @ step)
    n = im["H"] * im["W"]
    clouds = np.zeros((frames, n, 3), dtype=np.float32)
    for k, Wd in enumerate(world):
        d = beams(im, r.uniform(-0.3, 0.3, (n, 2)))
        dw = d @ Wd[:3, :3].T
        with np.errstate(divide="ignore"):
            t = np.where(dw > 0, (icp.ROOM - Wd[:3, 3]) / dw, (-icp.ROOM - Wd[:3, 3]) / dw)
        rng = t.min(axis=1) + r.normal(0.0, noise, n)
        pts = (d * rng[:, None]).astype(np.float32)
        margin = pixels(pts, im)[4]
        pts[margin < band] = 0.0
        clouds[k] = pts
    T = np.stack([np.eye(4)] + [np.linalg.inv(world[k - 1]) @ world[k] for k in range(1, frames)])
    return clouds, T
