"""The cases of tests/test_gpu_voxel_map_edges.py with their inputs, shared with tests/test_voxel_map_cases_cpu.py, which
proves on the model alone (tests/voxel_map_model.py) that every case reaches the edge it names and tells the model from
each of its planted faults.  CPU NumPy only.

A scenario is a dict: ``edge`` (the name of the edge), ``extent``, ``voxel``, ``frames`` (a list of dict(cloud (S, n, 3)
fp32, normals (S, n, 3) fp32, W (S, 4, 4) fp64: the pose every stream's frame is inserted with)) and ``queries`` (S, m, 3)
fp32 in the map frame, looked up after the last frame.  ``model_frames`` walks one through ``Grid``.  The begin, gate and
accumulate cases carry their own fields (see their builders).

Exactness.  Wherever a bound is asserted bit for bit the poses are translations and quarter turns about z whose entries
and products are exact in fp64, and the clouds are ``w - t`` for the fp32 value ``w`` that is wanted in the map frame;
``_exact32`` asserts that the difference is an fp32 number, so fp32(W p) IS w.
"""
import itertools

import numpy as np

import icp_model as model
import voxel_map_model as vm

F32 = np.float32
ANISO = ((8, 12, 4), (12, 8, 6), (6, 4, 10))
VOXELS = (0.5, 1.0, 2.0)
H_LO, H_HI = -2 ** 21, 2 ** 21 - 1                  # the ends of the storable half index
TINY = np.array([1], dtype=np.uint32).view(np.float32)[0]       # the smallest subnormal


def ext_id(extent):
    return "x".join(str(v) for v in extent)


def reach(extent, voxel):
    """(3,) fp64: the box rule's bound (N_a / 2 - 1) voxel."""
    return (np.asarray(extent) // 2 - 1).astype(np.float64) * float(voxel)


def quarter(turns, t):
    """A rotation by ``turns`` quarter turns about z, then the translation t: every entry exact."""
    c, s = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)][turns % 4]
    W = np.eye(4)
    W[:3, :3] = [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]
    W[:3, 3] = t
    return W


def inverse(W):
    """The inverse of a rigid pose."""
    V = np.eye(4)
    V[:3, :3] = W[:3, :3].T
    V[:3, 3] = -W[:3, :3].T @ W[:3, 3]
    return V


def _exact32(x):
    x = np.asarray(x, dtype=np.float64)
    y = x.astype(np.float32)
    assert np.array_equal(y.astype(np.float64), x), "not an fp32 value"
    return y


def cloud_for(W, w32):
    """The fp32 cloud whose image under the exact pose W is w32, bit for bit."""
    w = np.asarray(w32, dtype=np.float32)
    p = _exact32((w.astype(np.float64) - W[:3, 3]) @ W[:3, :3])
    assert np.array_equal(vm.to32(vm.pose_apply(W, p)).view(np.int32), w.view(np.int32))
    return p


def unit_normals(r, shape):
    nrm = r.normal(size=tuple(shape) + (3,))
    return (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(np.float32)


def scenario(edge, extent, voxel, frames, queries=None, **more):
    for f in frames:
        f["cloud"] = np.ascontiguousarray(f["cloud"], dtype=np.float32)
        f["normals"] = np.ascontiguousarray(f["normals"], dtype=np.float32)
        f["W"] = np.ascontiguousarray(f["W"], dtype=np.float64)
        assert f["cloud"].shape == f["normals"].shape and f["cloud"].shape[1] <= 600 and len(frames) <= 4
    return dict(dict(edge=edge, extent=tuple(extent), voxel=float(voxel), frames=frames,
                     queries=None if queries is None else np.ascontiguousarray(queries, dtype=np.float32)), **more)


def model_frames(sc, make=vm.Grid):
    """Walks a scenario through the model: yields (k, grids, slot (S, n), coord words before the frame (S, cells)) after
    every frame.  ``make``: the grid class (``planted(fault)`` for a faulty one).  The model's own check that no two voxels
    of a frame share a cell runs on every frame."""
    S = sc["frames"][0]["cloud"].shape[0]
    grids = [make(sc["extent"], sc["voxel"]) for _ in range(S)]
    for k, f in enumerate(sc["frames"]):
        before = np.stack([g.coord.copy() for g in grids])
        slots = []
        for s, g in enumerate(grids):
            _, slot, want = g.slots(f["cloud"][s], f["W"][s])
            assert make is not vm.Grid or vm.frame_voxels_share_no_cell(slot, want), (sc["edge"], k, s)
            slots.append(g.insert(f["cloud"][s], f["normals"][s], f["W"][s]))
            g.seq += 1
            g.nonempty, g.P = 1, f["W"][s].copy()
        yield k, grids, np.stack(slots), before


def model_end(sc, make=vm.Grid):
    """-> (grids after the last frame, the slots of every frame, the lookup of the queries per stream or None)."""
    slots, grids = [], None
    for _, grids, slot, _ in model_frames(sc, make):
        slots.append(slot)
    looks = None if sc["queries"] is None else [g.lookup(sc["queries"][s]) for s, g in enumerate(grids)]
    return grids, slots, looks


# ---- planted faults ----------------------------------------------------------------------------------------------------------

FAULTS = ("insert_cell_xy", "lookup_cell_xy", "box_le", "tie_le", "no_range")


def device_pack(v):
    """vm_pack for ANY int coordinate, as the device computes it: (unsigned)(c + 2^20) widened to 64 bits, shifted and or'd.
    A coordinate outside [-2^20, 2^20) spills into its neighbour's field, and a spilt word can equal a stored voxel's."""
    u = ((np.asarray(v, dtype=np.int64) + vm.BIAS) & 0xFFFFFFFF).astype(np.uint64)
    w = (u[..., 2] << np.uint64(42)) | (u[..., 1] << np.uint64(21)) | u[..., 0]
    return w.view(np.int64)


def planted(fault):
    """A Grid class with one line of the kernels' logic changed."""
    assert fault in FAULTS

    class Planted(vm.Grid):
        def _cell_xy(self, c):
            N = self.extent
            c = np.asarray(c, dtype=np.int64)
            return (np.mod(c[..., 2], N[2]) * N[0] + np.mod(c[..., 1], N[1])) * N[1] + np.mod(c[..., 0], N[0])

        def slots(self, cloud, W):
            w = vm.to32(vm.pose_apply(W, cloud))
            h, ok = vm.half_index(w, self.voxel)
            with np.errstate(invalid="ignore"):
                ok &= np.isfinite(w).all(axis=1)
                d = np.abs(w.astype(np.float64) - W[:3, 3])
                ok &= ((d <= reach(self.extent, self.voxel)) if fault == "box_le" else
                       (d < reach(self.extent, self.voxel))).all(axis=1)
            c = h >> 1
            octant = ((h[:, 2] & 1) << 2) | ((h[:, 1] & 1) << 1) | (h[:, 0] & 1)
            cell = self._cell_xy(c) if fault == "insert_cell_xy" else self.cell(c)
            return w, np.where(ok, cell * 8 + octant, -1), np.where(ok, vm.pack(c), vm.EMPTY)

        def lookup(self, q32):
            q = np.asarray(q32, dtype=np.float32)
            h, ok = vm.half_index(q, self.voxel)
            c = h >> 1
            best, bd = np.full((q.shape[0],), -1, dtype=np.int64), np.full((q.shape[0],), np.inf, dtype=np.float32)
            for dz, dy, dx in itertools.product((-1, 0, 1), repeat=3):
                v = c + np.array([dx, dy, dz])
                cell = self._cell_xy(v) if fault == "lookup_cell_xy" else self.cell(v)
                inside = ((v >= -vm.BIAS) & (v < vm.BIAS)).all(axis=1)
                if fault == "no_range":
                    inside[:] = True
                if (cell >= len(self.coord)).any():
                    raise IndexError("the faulty index leaves the grid")
                hit = ok & inside & (self.coord[cell] == device_pack(v))
                for o in range(8):
                    e = q - self.points[cell, o]
                    with np.errstate(invalid="ignore", over="ignore"):
                        d = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2], dtype=np.float32)
                        nearer = (d <= bd) if fault == "tie_le" else (d < bd)
                    take = hit & (self.keys[cell, o] != vm.EMPTY) & ((best < 0) | nearer)
                    best, bd = np.where(take, cell * 8 + o, best), np.where(take, d, bd)
            return np.where(best < 0, -1, best >> 3), np.where(best < 0, -1, best & 7), bd

    return Planted


def differs(sc, fault):
    """Whether the planted fault changes anything the GPU test compares for this scenario (slots, grids, lookups).  A faulty
    index that leaves the grid counts: on the device it would be an access out of bounds."""
    a = model_end(sc)
    try:
        b = model_end(sc, planted(fault))
    except IndexError:
        return True
    if any(not np.array_equal(x, y) for x, y in zip(a[1], b[1])):
        return True
    for g, f in zip(a[0], b[0]):
        if any(not np.array_equal(getattr(g, k).view(np.int64 if k in ("coord", "keys") else np.int32),
                                  getattr(f, k).view(np.int64 if k in ("coord", "keys") else np.int32))
               for k in ("coord", "keys", "points", "normals")):
            return True
    if a[2] is not None:
        for x, y in zip(a[2], b[2]):
            if not (np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and
                    np.array_equal(x[2].view(np.int32), y[2].view(np.int32))):
                return True
    return False


# ---- queries around what a grid holds ----------------------------------------------------------------------------------------

def queries_around(grids, sc_extent, voxel, m, seed):
    """(S, m, 3): stored points plus noise; every 7th one torus period away along x, y, z in turn (the cell aliases, the voxel
    differs); every 7th + 1 far from everything; NaN, -Inf and 3e38 rows; one stored point itself."""
    r = np.random.default_rng([seed, m])
    q = np.empty((len(grids), m, 3), dtype=np.float32)
    for s, g in enumerate(grids):
        pts = g.map_points()["points"]
        base = pts[r.integers(0, len(pts), m)]
        q[s] = base + r.normal(0.0, 0.3 * voxel, (m, 3)).astype(np.float32)
        for j in range(0, m, 7):
            a = (j // 7) % 3
            q[s, j, a] += F32(sc_extent[a] * voxel) * (1 if (j // 21) % 2 else -1)
        q[s, 1::7] = base[1::7] + F32(400.0 * voxel)
        if m > 12:
            q[s, 2], q[s, 3], q[s, 4] = [np.nan, 0, 0], [0, -np.inf, 0], [3e38, 0, 0]
            q[s, 9] = base[9]
    return q


# ---- 1. anisotropic extents ----------------------------------------------------------------------------------------------------

def aniso_walk(extent, voxel, n=300, frames=4, S=2):
    """A walk with a small yaw along a diagonal; the cloud's spread on every axis is 1.3 times that axis's own reach, so every
    axis rejects rows of its own."""
    rc = reach(extent, voxel)
    out = []
    for k in range(frames):
        r = np.random.default_rng([31, k, n])
        cloud = (r.uniform(-1.3, 1.3, (S, n, 3)) * rc).astype(np.float32)
        cloud[:, 5], cloud[:, 6] = [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0]
        W = np.stack([model.pose(model.rot([0.0, 0.1, 1.0], 0.02 * k + 0.3 * s), 0.45 * rc * k * [1, -1, 1][s % 3])
                      for s in range(S)])
        out.append(dict(cloud=cloud, normals=unit_normals(r, (S, n)), W=W))
    sc = scenario("anisotropic extent", extent, voxel, out)
    sc["queries"] = queries_around(model_end(sc)[0], extent, voxel, n, 5)
    return sc


# ---- 2. wraps ------------------------------------------------------------------------------------------------------------------

DIRECTIONS = {"-x": (-1, 0, 0), "+y": (0, 1, 0), "-y": (0, -1, 0), "+z": (0, 0, 1), "-z": (0, 0, -1), "-x+y-z": (-1, 1, -1)}


def wrap_walk(extent, voxel, direction, n=300):
    """Four frames whose sensor moves N_a / 2 + 1 voxels per frame along ``direction`` (more than half a period): pure
    translations, every row within the box."""
    d = np.asarray(DIRECTIONS[direction], dtype=np.float64)
    step = d * (np.asarray(extent) // 2 + 1) * voxel
    rc = reach(extent, voxel)
    out = []
    for k in range(4):
        r = np.random.default_rng([41, k, n])
        cloud = (r.uniform(-0.98, 0.98, (1, n, 3)) * rc).astype(np.float32)
        out.append(dict(cloud=cloud, normals=unit_normals(r, (1, n)), W=quarter(0, step * k)[None]))
    sc = scenario("wrap " + direction, extent, voxel, out, direction=tuple(int(v) for v in d))
    grids = model_end(sc)[0]
    q = queries_around(grids, extent, voxel, n, 6)
    first = vm.to32(vm.pose_apply(out[0]["W"][0], out[0]["cloud"][0]))     # where frame 0 was: evicted or still there
    q[0, 20:120] = first[20:120]
    sc["queries"] = q
    return sc


# ---- 3. the ends of the packed range ---------------------------------------------------------------------------------------------

def range_end(extent, voxel, end, axes):
    """One frame whose sensor sits on the ``end`` ("low" / "high") of the packed range on ``axes`` and at 0 on the others.
    Rows: every combination, per end axis, of the two storable half indices next to the end and the one beyond it, each on
    the octant's boundary and in its middle; on the other axes the middles of h = -2 .. 1.  -> scenario with ``stored`` (n,)
    bool, ``h`` (n, 3) the half indices asked for, and queries: every row itself, a quarter octant off, and the same rows
    moved to the opposite end of the range, where only a coordinate out of range could alias onto them."""
    half = voxel / 2
    hs = (H_LO, H_LO + 1, H_LO - 1) if end == "low" else (H_HI - 1, H_HI, H_HI + 1)
    t = np.array([(H_LO if end == "low" else H_HI) * half if a in axes else 0.0 for a in range(3)])
    per_axis = []
    for a in range(3):
        if a in axes:
            per_axis.append([(h, h * half + off) for h in hs for off in (0.0, half / 2)])
        else:
            per_axis.append([(h, h * half + half / 2) for h in (-2, -1, 0, 1)])
    rows = list(itertools.product(*per_axis))
    h = np.array([[v[0] for v in row] for row in rows], dtype=np.int64)
    w = _exact32(np.array([[v[1] for v in row] for row in rows]))
    W = quarter(0, t)
    cloud = cloud_for(W, w)
    r = np.random.default_rng([51, len(rows)])
    stored = ((h >= H_LO) & (h <= H_HI)).all(axis=1)
    far = w.astype(np.float64)                                            # the same rows at the opposite end of the range
    for a in axes:
        far[:, a] += (2.0 ** 21 - 1) * voxel * (1 if end == "low" else -1)
    q = np.concatenate([w, _exact32(w.astype(np.float64) + half / 4), _exact32(far)])[None]
    return scenario("range end %s %s" % (end, "xyz"[axes[0]] if len(axes) == 1 else "corner"), extent, voxel,
                    [dict(cloud=cloud[None], normals=unit_normals(r, (1, len(rows))), W=W[None])], q, stored=stored, h=h,
                    axes=tuple(axes), end=end)


ZERO_VALUES = lambda voxel: np.array([TINY, -TINY, 1e-30, -1e-30, -voxel / 2, -voxel, -0.0, 0.0, voxel / 2], dtype=np.float32)


def zero_straddle(extent, voxel):
    """Rows around 0 on every axis, sensor at the origin: +-the smallest subnormal, +-1e-30, -half, -voxel, -0.0, 0.0, +half.
    Every pair of values occurs on every pair of axes (the triples whose index sum is even)."""
    vals = ZERO_VALUES(voxel)
    idx = np.array([ijk for ijk in itertools.product(range(len(vals)), repeat=3) if sum(ijk) % 2 == 0])
    w = vals[idx]
    r = np.random.default_rng([52, len(w)])
    q = np.concatenate([w, w + F32(voxel / 8)])[None]
    return scenario("zero straddle", extent, voxel,
                    [dict(cloud=w[None], normals=unit_normals(r, (1, len(w))), W=np.eye(4)[None])], q, idx=idx)


# ---- 4. the box rule at its bound ------------------------------------------------------------------------------------------------

BOUND_T = np.array([96.25, -160.5, 64.75])          # |t_a| >= 4 bound_a + ...: fp32 is no finer at t +- bound than at the bound


def box_bound(extent, voxel, turns, n=300):
    """One frame, pose = ``turns`` quarter turns about z then the translation BOUND_T.  For every axis and sign three rows whose
    map-frame coordinate on that axis is w0 = fp32(t + sign bound) and its two fp32 neighbours, with the other two coordinates
    inside the box; the eight corners at the inner neighbours; filler inside the box.  -> ``kind`` (n,): 0 filler, 1 the inner
    neighbour (stored), 2 the bound, 3 the outer neighbour (both refused), ``axis`` and ``sign`` (n,)."""
    rc = reach(extent, voxel)
    W = quarter(turns, BOUND_T)
    r = np.random.default_rng([61, turns, n])
    w = _exact32(BOUND_T + np.trunc(r.uniform(-0.9, 0.9, (n, 3)) * rc * 8) / 8)
    kind, axis, sign = np.zeros((n,), dtype=int), np.full((n,), -1), np.zeros((n,), dtype=int)
    at = lambda a, sg, k: [None, np.nextafter(F32(BOUND_T[a] + sg * rc[a]), F32(BOUND_T[a])), F32(BOUND_T[a] + sg * rc[a]),
                           np.nextafter(F32(BOUND_T[a] + sg * rc[a]), F32(sg * np.inf))][k]
    special = [0, 255, 256, n - 1]                                       # the launch's own edges carry bound rows too
    it = iter(special + [int(i) for i in r.permutation(n) if i not in special])
    for a in range(3):
        assert float(F32(BOUND_T[a] + rc[a])) == BOUND_T[a] + rc[a] and float(F32(BOUND_T[a] - rc[a])) == BOUND_T[a] - rc[a]
        for sg in (1, -1):
            for k in (1, 2, 3):
                i = next(it)
                w[i, a], kind[i], axis[i], sign[i] = at(a, sg, k), k, a, sg
    for corner in itertools.product((1, -1), repeat=3):
        i = next(it)
        w[i], kind[i] = [at(a, corner[a], 1) for a in range(3)], 1
    return scenario("box bound, %d quarter turns" % turns, extent, voxel,
                    [dict(cloud=cloud_for(W, w)[None], normals=unit_normals(r, (1, n)), W=W[None])], w[None].copy(),
                    kind=kind, axis=axis, sign=sign)


# ---- 5. exact ties ---------------------------------------------------------------------------------------------------------------

# name -> (the two stored points A and B and the query, in voxels from the base voxel's corner; A is first in (dz, dy, dx, octant)
# order and wins).  A decoy farther off shares the grid.
TIE_ARRANGEMENTS = {
    "octants x": ((.25, .25, .25), (.75, .25, .25), (.5, .25, .25)),
    "octants z": ((.25, .75, .25), (.25, .75, .75), (.25, .75, .5)),
    "cells dx": ((-.25, .25, .25), (.25, .25, .25), (0., .25, .25)),
    "cells dx, query in the lower": ((.5, .25, .25), (1., .25, .25), (.75, .25, .25)),
    "cells dy": ((.25, -.25, .75), (.25, .25, .75), (.25, 0., .75)),
    "cells dz, later one in a lower octant": ((.75, .75, -.25), (.75, .75, .25), (.75, .75, 0.)),
}
TIE_DECOY = (-.75, -.75, -.75)
TIE_BASES = ((1, 1, 1), (0, 0, 0))                  # (0, 0, 0): voxel -1 wraps to the last cell, so A has the HIGHER cell index


def ties(extent, voxel):
    """One stream per (arrangement, base): rows A, B (B first in the cloud for the odd streams, so neither the row nor the key
    decides), a decoy and a refused NaN row; the sensor sits on the base voxel's corner.  -> ``names`` and, per stream, the
    rows of A and B."""
    clouds, Ws, qs, names, ab = [], [], [], [], []
    for s, ((name, (A, B, Q)), base) in enumerate(itertools.product(TIE_ARRANGEMENTS.items(), TIE_BASES)):
        t = np.asarray(base, dtype=np.float64) * voxel
        W = quarter(0, t)
        rows = [A, B] if s % 2 == 0 else [B, A]
        w = _exact32(np.array(rows + [TIE_DECOY]) * voxel + t)
        clouds.append(np.concatenate([cloud_for(W, w), F32([[np.nan, 0, 0]])]))
        Ws.append(W)
        qs.append(_exact32(np.array([Q]) * voxel + t))
        names.append("%s at %s" % (name, base))
        ab.append((0, 1) if s % 2 == 0 else (1, 0))
    r = np.random.default_rng(71)
    return scenario("exact ties", extent, voxel, [dict(cloud=np.stack(clouds), normals=unit_normals(r, (len(Ws), 4)),
                                                        W=np.stack(Ws))], np.stack(qs), names=names, ab=ab)


def tie_candidates(grid, q):
    """The second derivation: every stored entry of the 27 voxels around q as (fp32 distance bits, dz, dy, dx, octant, cell),
    sorted.  The winner is the first row."""
    q = np.asarray(q, dtype=np.float32)
    c = vm.half_index(q[None], grid.voxel)[0][0] >> 1
    rows = []
    for dz, dy, dx in itertools.product((-1, 0, 1), repeat=3):
        v = c + np.array([dx, dy, dz])
        cell = int(grid.cell(v))
        if grid.coord[cell] != vm.pack(v):
            continue
        for o in range(8):
            if grid.keys[cell, o] != vm.EMPTY:
                e = q - grid.points[cell, o]
                d = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2], dtype=np.float32)
                rows.append((int(F32(d).view(np.int32)), dz, dy, dx, o, cell))
    return sorted(rows)


# ---- 6. the first point stays ----------------------------------------------------------------------------------------------------

DUPLICATES = ((0, 255, 256, 299), (255, 256, 299), (256, 299))


def first_point_stays(extent, voxel, n=300):
    """Two frames with the same pose, three streams.  Frame 0 (seq 0) fills octants whose half indices have an even sum;
    frame 1 (seq 1) aims at every octant of the same cells: occupied ones keep their bits, empty ones are filled.  A row's
    place inside its octant depends on the row, so the stored bits name the row that won.  Stream s repeats one octant in the
    rows DUPLICATES[s] of both frames."""
    half = voxel / 2
    lim = (np.asarray(extent) // 2 - 1) * 2                               # h in [-lim, lim)
    W = quarter(1, [2.0 * voxel, -1.0 * voxel, 3.0 * voxel])
    frames = []
    for k in range(2):
        r = np.random.default_rng([81, k, n])
        h = r.integers(-lim, lim, (3, n, 3))
        if k == 0:
            h[..., 0] -= (h.sum(axis=-1) % 2) * np.where(h[..., 0] > -lim[0], 1, -1)       # make the sum even, stay inside
        for s, rows in enumerate(DUPLICATES):
            h[s, (h[s] == [1, -1, 0]).all(axis=1)] = [-1, 1, 0]            # the repeated octant is the repeated rows' alone
            h[s, list(rows)] = [1, -1, 0]
        off = (1 + np.arange(n) % 97)[None, :, None] / 128.0 + k / 256.0  # inside the octant, in half voxels: below 0.78
        w = _exact32((h + off) * half + W[:3, 3])
        frames.append(dict(cloud=np.stack([cloud_for(W, w[s]) for s in range(3)]), normals=unit_normals(r, (3, n)),
                           W=np.stack([W] * 3)))
    sc = scenario("first point stays", extent, voxel, frames)
    sc["queries"] = queries_around(model_end(sc)[0], extent, voxel, 64, 8)
    return sc


# ---- 7. begin --------------------------------------------------------------------------------------------------------------------

BEGIN_EXTENTS = ((4, 4, 4), (18, 16, 14), (18, 16, 16), (32, 32, 16))     # 64, 4032, 4608 and 16384 cells
# three launches of S = 3: every combination of (active, restart, armed), and armed on an idle stream twice
BEGIN_ROUNDS = (((0, 0, 0), (1, 0, 0), (1, 1, 0)), ((1, 0, 1), (1, 1, 1), (0, 1, 0)), ((0, 0, 1), (0, 1, 1), (1, 0, 5)))


def grid_bytes(grids):
    """The grid buffer of these streams, section by section, as the device lays it out."""
    parts = [np.stack([getattr(g, k) for g in grids]).reshape(-1).view(np.uint8) for k in ("coord", "keys", "points", "normals")]
    return np.concatenate(parts)


def begin_case(extent, rnd):
    """Sentinel bits everywhere -> dict(buffer (bytes,) uint8, P (3, 4, 4), nonempty (3, 1), seq (3,), active, restart, armed
    (3,) int32, and what begin must leave: ``want`` of the same names)."""
    S = 3
    cells = extent[0] * extent[1] * extent[2]
    r = np.random.default_rng([91, cells, rnd])
    grids = []
    for s in range(S):
        g = vm.Grid(extent, 1.0)
        g.coord = r.integers(0, 2 ** 62, (cells,), dtype=np.int64)
        g.keys = r.integers(0, 2 ** 40, (cells, 8), dtype=np.int64)
        g.points = r.normal(size=(cells, 8, 3)).astype(np.float32)
        g.normals = r.normal(size=(cells, 8, 3)).astype(np.float32)
        g.P, g.nonempty, g.seq = r.normal(size=(4, 4)), 1 + s, 1000 + s
        grids.append(g)
    masks = np.array(BEGIN_ROUNDS[rnd], dtype=np.int32)
    case = dict(edge="begin %s round %d" % (ext_id(extent), rnd), extent=extent, buffer=grid_bytes(grids),
                P=np.stack([g.P for g in grids]), nonempty=np.array([[g.nonempty] for g in grids], dtype=np.int32),
                seq=np.array([g.seq for g in grids], dtype=np.int32), active=masks[:, 0].copy(), restart=masks[:, 1].copy(),
                armed=masks[:, 2].copy())
    cleared = [vm.masked_begin(g, *masks[s]) for s, g in enumerate(grids)]
    case["want"] = dict(buffer=grid_bytes(grids), P=np.stack([g.P for g in grids]),
                        nonempty=np.array([[g.nonempty] for g in grids], dtype=np.int32),
                        seq=np.array([g.seq for g in grids], dtype=np.int32), armed=masks[:, 2].copy())
    case["cleared"] = cleared
    return case


# ---- 8. pose and gates -----------------------------------------------------------------------------------------------------------

GATE_S = (1, 63, 64, 65, 1024)
GATE_EXTENT, GATE_VOXEL, GATE_N = (6, 4, 10), 1.0, 40
# which optional arguments a launch gets
GATE_CONFIGS = (dict(T=False, nonempty=True, active=True, insert=True), dict(T=True, nonempty=True, active=True, insert=True),
                dict(T=True, nonempty=False, active=True, insert=True), dict(T=True, nonempty=True, active=False, insert=True),
                dict(T=True, nonempty=True, active=True, insert=False), dict(T=False, nonempty=False, active=False, insert=False))


def gate_case(S):
    """Per stream: active = not bit 0 of s, insert = not bit 1, nonempty = not bit 2 (every combination occurs from S = 8 on;
    the one stream of S = 1 does everything), armed words 0, 1 and -7, P a quarter turn and translation, T a general small
    motion, seq = s % 5 before ``prefill``, a frame every stream inserted before with its P in lock step (seq + 1 after)."""
    s = np.arange(S)
    r = np.random.default_rng([101, S])
    rc = reach(GATE_EXTENT, GATE_VOXEL)
    P = np.stack([quarter(int(i) % 4, np.round(r.uniform(-20, 20, 3) * 4) / 4) for i in s])
    T = np.stack([model.pose(model.rot(r.normal(size=3), r.uniform(0, 0.1)), r.uniform(-0.5, 0.5, 3)) for _ in s])
    small = min(S, 65)                                                     # clouds only where a grid is run
    mk = lambda seed: (np.random.default_rng([102, seed, S]).uniform(-1.2, 1.2, (small, GATE_N, 3)) * rc).astype(np.float32)
    return dict(edge="gates S=%d" % S, S=S, extent=GATE_EXTENT, voxel=GATE_VOXEL, P=P, T=T,
                active=(1 - (s & 1)).astype(np.int32) * 3, insert=(1 - ((s >> 1) & 1)).astype(np.int32) * 2,
                nonempty=(1 - ((s >> 2) & 1)).astype(np.int32)[:, None].copy(), seq=(s % 5).astype(np.int32),
                armed=np.array([0, 1, -7], dtype=np.int32)[s % 3].copy(), with_grid=S <= 65,
                prefill=dict(cloud=mk(0), normals=unit_normals(r, (small, GATE_N))),
                frame=dict(cloud=mk(1), normals=unit_normals(r, (small, GATE_N))))


def gate_model(case, cfg):
    """-> (grids or None, slot (S, n) or None with -1 rows where a stream did not insert, P, nonempty, seq, armed) after
    ``insert`` and ``pose`` with the optional arguments of ``cfg``."""
    S = case["S"]
    ext = case["extent"] if case["with_grid"] else (4, 4, 4)
    grids, slot = [], np.full((S, GATE_N), -1, dtype=np.int32)
    armed = case["armed"].copy()
    for s in range(S):
        g = vm.Grid(ext, case["voxel"])
        g.P, g.seq = case["P"][s].copy(), int(case["seq"][s])
        if case["with_grid"]:
            g.insert(case["prefill"]["cloud"][s], case["prefill"]["normals"][s], g.P)
        g.seq += 1
        g.nonempty = int(case["nonempty"][s, 0])
        T = case["T"][s] if cfg["T"] else None
        a = case["active"][s] if cfg["active"] else 1
        i = case["insert"][s] if cfg["insert"] else 1
        if case["with_grid"]:
            got = vm.masked_insert(g, case["frame"]["cloud"][s], case["frame"]["normals"][s], T, cfg["nonempty"], a, i)
            if got is not None:
                slot[s] = got
        armed[s] = vm.masked_pose(g, T, armed[s], a, i)
        grids.append(g)
    return (grids if case["with_grid"] else None, slot if case["with_grid"] else None, np.stack([g.P for g in grids]),
            np.array([[g.nonempty] for g in grids], dtype=np.int32), np.array([g.seq for g in grids], dtype=np.int32), armed)


# ---- 9. accumulate shapes --------------------------------------------------------------------------------------------------------

ACC_N = (1, 255, 256, 257, 513)
ACC_SPECIAL = (0, 255, 256, 511, 512)               # first and last rows of workgroups
ACC_POISON = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [3e38, 3e38, 0]]
ACC_P = quarter(1, [3.0, -2.0, 1.0])
ACC_TQ = quarter(3, [0.5, 0.25, -0.25])
ACC_TG = model.pose(model.rot([0.3, -0.2, 1.0], 0.05), [0.1, -0.05, 0.02])
SIGMA = 0.5


def max_dists(voxel):
    return (0.0, voxel / 4, voxel)


def accumulate_case(extent, voxel, n):
    """A grid of 200 points on a lattice of voxel / 32 (stream 1 holds the same), the first of them with a zero normal, and
    n query rows per variant of T (None, a quarter turn, a general motion): row 1 sits on the zero-normal point, every fourth
    row on a stored point (the two exact variants: bit for bit, d = 0), the others up to 1.5 voxels off; the rows ACC_SPECIAL
    (from n = 255 on) and n - 1 are NaN, +-Inf and 3e38.  Stream 1 is idle and its p is NaN."""
    rc = reach(extent, voxel)
    r = np.random.default_rng([111, n])
    lat = voxel / 32
    w = _exact32(ACC_P[:3, 3] + np.round(r.uniform(-0.95, 0.95, (200, 3)) * rc / lat) * lat)
    nrm = unit_normals(r, (200,))
    nrm[0] = 0.0
    frame = dict(cloud=np.stack([cloud_for(ACC_P, w)] * 2), normals=np.stack([nrm] * 2), W=np.stack([ACC_P] * 2))
    sc = scenario("accumulate n=%d" % n, extent, voxel, [frame])
    g = model_end(sc)[0][0]
    pts = g.map_points()
    zero = int(np.flatnonzero((pts["normals"] == 0).all(axis=1))[0])
    j = r.integers(0, len(pts["keys"]), n)
    off = np.round(r.uniform(-1.5, 1.5, (n, 3)) * voxel / np.sqrt(3) / lat) * lat
    off[r.random(n) < 0.5] /= 4
    off[0::4] = 0.0
    if n > 1:
        j[1], off[1] = zero, 0.0
    elif j[0] == zero:
        j[0] = (zero + 1) % len(pts["keys"])
    q = _exact32(pts["points"][j].astype(np.float64) + off)
    poison = [i for i in sorted(set(ACC_SPECIAL + (n - 1,))) if i < n] if n >= 255 else []
    variants = {}
    for name, T in (("none", None), ("quarter", ACC_TQ), ("general", ACC_TG)):
        M = ACC_P if T is None else vm.pose_mul(ACC_P, T)
        p = cloud_for(M, q) if name != "general" else vm.to32(vm.pose_apply(inverse(M), q))
        for c, i in enumerate(poison):
            p[i] = ACC_POISON[c % 4]
        variants[name] = (T, np.stack([p, np.full_like(p, np.nan)]))
    sc.update(variants=variants, P=np.stack([ACC_P, ACC_P]), active=np.array([1, 0], dtype=np.int32), poison=poison,
              zero_row=1 if n > 1 else None, n=n)
    return sc
