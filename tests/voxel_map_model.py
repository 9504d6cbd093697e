"""NumPy model of the persistent voxel map of csrc/voxel_map.hpp / voxel_map.hip: the toroidal grid,
insertion, implicit eviction, the 27-voxel lookup and the registration, in the kernels' own order of operations -- fp64
products added in the order of icp.hpp, one rounding to fp32, fp32 distances -- so that grids, lookups and distances are
the device's bit for bit.  The weights, the rows' layout and the solve are icp_model's."""
import numpy as np

import icp_model as model

BIAS = 1 << 20
EMPTY = -1                                       # all ones, read as int64
H_LIMIT = 2097152.0                              # 2^21: a coordinate is storable where -2^21 <= h < 2^21


# ---- icp.hpp's products, in its order ------------------------------------------------------------------------------------------

def pose_mul(a, b):
    """icp_pose_mul: (a0 b0 + a1 b1) + a2 b2, the translation added last."""
    c = np.eye(4)
    for i in range(3):
        for j in range(4):
            s = (a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j]
            c[i, j] = s + a[i, 3] if j == 3 else s
    return c


def pose_apply(a, p32):
    """icp_pose_apply on (n, 3) fp32 -> (n, 3) fp64."""
    p = np.asarray(p32, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):                      # Inf coordinates give NaN products, as on the device
        return np.stack([((a[i, 0] * p[:, 0] + a[i, 1] * p[:, 1]) + a[i, 2] * p[:, 2]) + a[i, 3] for i in range(3)], axis=1)


def rotate(a, n32):
    n = np.asarray(n32, dtype=np.float32).astype(np.float64)
    return np.stack([(a[i, 0] * n[:, 0] + a[i, 1] * n[:, 1]) + a[i, 2] * n[:, 2] for i in range(3)], axis=1)


def to32(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x).astype(np.float32)


# ---- coordinates -------------------------------------------------------------------------------------------------------------------

def half_index(w32, voxel):
    """(n, 3) fp32 -> (h (n, 3) int64, ok (n,)): h_a = floor((double)w_a / (voxel / 2)); ok where every axis is storable."""
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(np.asarray(w32, dtype=np.float32).astype(np.float64) / (float(voxel) / 2))
        ok = ((f >= -H_LIMIT) & (f < H_LIMIT)).all(axis=1)
    return np.where(ok[:, None], f, 0.0).astype(np.int64), ok


def pack(c):
    c = np.asarray(c, dtype=np.int64)
    return ((c[..., 2] + BIAS) << 42) | ((c[..., 1] + BIAS) << 21) | (c[..., 0] + BIAS)


def unpack(word):
    w = np.asarray(word, dtype=np.int64)
    return np.stack([(w & 0x1FFFFF) - BIAS, ((w >> 21) & 0x1FFFFF) - BIAS, ((w >> 42) & 0x1FFFFF) - BIAS], axis=-1)


class Grid:
    """One stream's map: coord (cells,), keys (cells, 8) int64 (-1: empty), points and normals (cells, 8, 3) fp32, and the
    words beside it: P (4, 4), nonempty, seq."""

    def __init__(self, extent=(128, 128, 32), voxel=1.0):
        self.extent, self.voxel = tuple(int(v) for v in extent), float(voxel)
        assert all(v >= 4 and v % 2 == 0 for v in self.extent)
        cells = self.extent[0] * self.extent[1] * self.extent[2]
        self.coord = np.full((cells,), EMPTY, dtype=np.int64)
        self.keys = np.full((cells, 8), EMPTY, dtype=np.int64)
        self.points = np.zeros((cells, 8, 3), dtype=np.float32)
        self.normals = np.zeros((cells, 8, 3), dtype=np.float32)
        self.P, self.nonempty, self.seq = np.eye(4), 0, 0

    def begin(self):
        """A restart: coordinate words only (a stale cell's keys are emptied when a voxel claims it)."""
        self.coord[:] = EMPTY
        self.P, self.nonempty, self.seq = np.eye(4), 0, 0

    def cell(self, c):
        N = self.extent
        c = np.asarray(c, dtype=np.int64)
        return (np.mod(c[..., 2], N[2]) * N[1] + np.mod(c[..., 1], N[1])) * N[0] + np.mod(c[..., 0], N[0])

    # ---- insertion ---------------------------------------------------------------------------------------------------------------

    def slots(self, cloud, W):
        """-> (w (n, 3) fp32 = fp32(W p), slot (n,) = cell * 8 + octant or -1, want (n,) the voxel's word)."""
        w = to32(pose_apply(W, cloud))
        h, ok = half_index(w, self.voxel)
        with np.errstate(invalid="ignore"):
            ok &= np.isfinite(w).all(axis=1)
            reach = (np.asarray(self.extent) // 2 - 1).astype(np.float64) * self.voxel
            ok &= (np.abs(w.astype(np.float64) - W[:3, 3]) < reach).all(axis=1)
        c = h >> 1
        octant = ((h[:, 2] & 1) << 2) | ((h[:, 1] & 1) << 1) | (h[:, 0] & 1)
        return w, np.where(ok, self.cell(c) * 8 + octant, -1), np.where(ok, pack(c), EMPTY)

    def insert(self, cloud, normals32, W, order=None):
        """The four phases, each walked point by point in ``order`` (any permutation gives the same map).  -> slot (n,)."""
        cloud = np.asarray(cloud, dtype=np.float32)
        n = cloud.shape[0]
        order = np.arange(n) if order is None else np.asarray(order)
        w, slot, want = self.slots(cloud, W)
        nw = to32(rotate(W, normals32))
        stale = set()
        for i in order:                                      # 1: claim and mark
            if slot[i] >= 0 and self.coord[slot[i] >> 3] != want[i]:
                self.coord[slot[i] >> 3] = want[i]
                stale.add(int(slot[i] >> 3))
        for cell in stale:                                   # 2: empty the marked cells' keys
            self.keys[cell] = EMPTY
        for i in order:                                      # 3: the smallest key stands
            if slot[i] >= 0:
                key, old = (self.seq << 32) | int(i), self.keys[slot[i] >> 3, slot[i] & 7]
                if old == EMPTY or key < old:
                    self.keys[slot[i] >> 3, slot[i] & 7] = key
        for i in order:                                      # 4: its row writes
            if slot[i] >= 0 and self.keys[slot[i] >> 3, slot[i] & 7] == ((self.seq << 32) | int(i)):
                self.points[slot[i] >> 3, slot[i] & 7] = w[i]
                self.normals[slot[i] >> 3, slot[i] & 7] = nw[i]
        return slot

    def push(self, cloud, normals32, T, insert=True):
        """The pose and insertion launches of one ``register``: W = I for an empty map, else P T."""
        W = np.eye(4) if not self.nonempty else pose_mul(self.P, np.asarray(T, dtype=np.float64))
        slot = self.insert(cloud, normals32, W) if insert else None
        self.P = W
        if insert:
            self.seq += 1
            self.nonempty = 1
        return slot

    def map_points(self):
        """As VoxelMapRefiner.map_points: the entries whose cell has an owner and whose key is not empty, in cell and octant
        order."""
        keep = (self.coord != EMPTY)[:, None] & (self.keys != EMPTY)
        cell, octant = np.nonzero(keep)
        return dict(points=self.points[cell, octant], normals=self.normals[cell, octant], voxels=unpack(self.coord[cell]),
                    octants=octant, keys=self.keys[cell, octant], cells=cell)

    # ---- lookup ------------------------------------------------------------------------------------------------------------------

    def lookup(self, q32):
        """q (n, 3) fp32 -> (cell, octant (n,) int, dist (n,) fp32): the nearest stored entry among the 27 voxels around q,
        candidates in the order dz, dy, dx, octant, strict <; -1, -1, +Inf where there is none."""
        q = np.asarray(q32, dtype=np.float32)
        n = q.shape[0]
        h, ok = half_index(q, self.voxel)
        c = h >> 1
        best, bd = np.full((n,), -1, dtype=np.int64), np.full((n,), np.inf, dtype=np.float32)
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    v = c + np.array([dx, dy, dz])
                    cell = self.cell(v)
                    hit = ok & ((v >= -BIAS) & (v < BIAS)).all(axis=1) & (self.coord[cell] == pack(v))
                    for o in range(8):
                        cand = hit & (self.keys[cell, o] != EMPTY)
                        e = q - self.points[cell, o]
                        with np.errstate(invalid="ignore", over="ignore"):
                            d = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2], dtype=np.float32)
                            take = cand & ((best < 0) | (d < bd))
                        best = np.where(take, cell * 8 + o, best)
                        bd = np.where(take, d, bd)
        return np.where(best < 0, -1, best >> 3), np.where(best < 0, -1, best & 7), bd

    def accumulate(self, p, T, sigma, max_dist, P=None):
        """One stream's row of sums -> (sum (32,), sum of |term| (32,), (cell, octant, dist))."""
        P = self.P if P is None else P
        p = np.asarray(p, dtype=np.float32)
        q = to32(pose_apply(pose_mul(P, T), p))
        cell, octant, dist = self.lookup(q)
        out, mag = np.zeros((model.ROW,)), np.zeros((model.ROW,))
        with np.errstate(invalid="ignore"):
            ok = (cell >= 0) & (dist <= np.float32(max_dist))
        ok &= (self.normals[np.maximum(cell, 0), np.maximum(octant, 0)] != 0).any(axis=1)
        sel = np.flatnonzero(ok)
        if sel.size:
            y = self.points[cell[sel], octant[sel]].astype(np.float64)
            nn = self.normals[cell[sel], octant[sel]].astype(np.float64)
            r = np.einsum("ni,ni->n", nn, q[sel].astype(np.float64) - y)
            npr = nn @ P[:3, :3]                             # R_P^T n: the map frame -> the previous frame
            pp = pose_apply(T, p[sel])
            J = np.concatenate([np.cross(pp, npr), npr], axis=1)
            w2 = model.huber_w2(r, sigma)
            for e, (a, b) in enumerate(model.UPPER):
                t = w2 * J[:, a] * J[:, b]
                out[model.H0 + e], mag[model.H0 + e] = t.sum(), np.abs(t).sum()
            for a in range(6):
                t = w2 * J[:, a] * r
                out[model.G0 + a], mag[model.G0 + a] = t.sum(), np.abs(t).sum()
            out[model.SW] = mag[model.SW] = w2.sum()
            out[model.COST] = mag[model.COST] = (w2 * r * r).sum()
            out[model.PAIRS] = mag[model.PAIRS] = float(sel.size)
        return out, mag, (cell, octant, dist)


def brute_nearest(grid, q32):
    """The distance to the nearest of ``grid.map_points()`` by exhaustive search, in the lookup's fp32 arithmetic."""
    pts = grid.map_points()["points"]
    q = np.asarray(q32, dtype=np.float32)
    if pts.shape[0] == 0:
        return np.full((q.shape[0],), np.inf, dtype=np.float32)
    e = q[:, None, :] - pts[None, :, :]
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2], dtype=np.float32)
    return np.fmin.reduce(d, axis=1)


def register(grid, cloud, init, normals32=None, iters=10, sigma=0.5, max_dist=1.0, damping=1e-6, threshold=1e-4,
             min_pairs=64, k=10, insert=True):
    """One ``VoxelMapRefiner.register`` of one stream -> (T, status, per-iteration dicts).  ``normals32``: the frame's
    normals as the device staged them (None: icp_model's, which agree up to the eigen-solver)."""
    T, status, steps = np.array(init, dtype=np.float64), 0, []
    cloud = np.asarray(cloud, dtype=np.float32)
    for it in range(iters):
        row, mag, near = grid.accumulate(cloud, T, sigma, max_dist)
        s = model.solve(row, T, status, it, damping, threshold, min_pairs)
        T, status = s["T"], s["status"]
        steps.append(dict(row=row, mag=mag, delta=s["delta"], T=T, status=status, near=near))
    if normals32 is None:
        normals32 = model.normals(cloud, k)[0].astype(np.float32)
    grid.push(cloud, normals32, T, insert)
    return T, status, steps


# ---- the stand-alone ops with their masks --------------------------------------------------------------------------------------------

def frame_voxels_share_no_cell(slot, want):
    """The invariant voxel_claim_kernel rests on: among the rows of one frame that are inserted, every cell is asked for by
    one voxel only.  slot, want: what ``Grid.slots`` returns."""
    slot, want = np.asarray(slot), np.asarray(want)
    kept = slot >= 0
    pairs = np.unique(np.stack([slot[kept] >> 3, want[kept]], axis=1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs)


def insert_pose(grid, T=None, use_nonempty=True):
    """vm_insert_pose: I for an empty map (where the nonempty word is passed), else P T, or P where no T is given."""
    if use_nonempty and not grid.nonempty:
        return np.eye(4)
    return grid.P.copy() if T is None else pose_mul(grid.P, np.asarray(T, dtype=np.float64))


def masked_begin(grid, active=1, restart=0, armed=0):
    """``voxel_map.begin`` for one stream: cleared where ``active and (restart or armed)``; armed is only read.
    -> whether the stream was cleared."""
    clear = bool(active) and (bool(restart) or bool(armed))
    if clear:
        grid.begin()
    return clear


def masked_insert(grid, cloud, normals32, T=None, use_nonempty=True, active=1, insert=1):
    """``voxel_map.insert`` for one stream -> slot (n,), or None where the stream does not insert (its slot rows are not
    written).  P, nonempty and seq stay: they are ``masked_pose``'s."""
    if not (bool(active) and bool(insert)):
        return None
    W = insert_pose(grid, T, use_nonempty)
    assert frame_voxels_share_no_cell(*grid.slots(cloud, W)[1:])
    return grid.insert(cloud, normals32, W)


def masked_pose(grid, T=None, armed=0, active=1, insert=1):
    """``voxel_map.pose`` for one stream -> the armed word afterwards."""
    if not bool(active):
        return armed
    grid.P = insert_pose(grid, T)
    if bool(insert):
        grid.seq += 1
        grid.nonempty = 1
    return 0


# ---- scenes --------------------------------------------------------------------------------------------------------------------------

def walk_clouds(seed, frames, n, step, spread):
    """Clouds for insertion tests: ``n`` points uniform within ``spread`` metres of a sensor that moves ``step`` metres per
    frame along x (and a little along y and z), with unit normals; poses are pure translations plus a small yaw.
    -> (clouds (frames, n, 3) fp32 in the sensor frames, normals (frames, n, 3) fp32, poses (frames, 4, 4) absolute)."""
    r = np.random.default_rng([seed, frames, n])
    clouds = r.uniform(-spread, spread, (frames, n, 3)).astype(np.float32)
    nrm = r.normal(size=(frames, n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(np.float32)
    poses = np.stack([model.pose(model.rot([0.0, 0.1, 1.0], 0.02 * k), [step * k, 0.13 * k, -0.07 * k]) for k in range(frames)])
    return clouds, nrm, poses
