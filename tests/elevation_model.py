"""NumPy model of the loop detector's translation search ("Translation on elevation grids"): the
specification restated, not the kernels' code.

Between Scan Context's select and the verifying registration the detector images the matched place's stored cloud (E) and the
query under Y yaw candidates (Q_k) as G x G grids of 8-bit height levels, scores every planar offset (a, b) in [-W, W]^2 of
every candidate by an integer agreement sum, and seeds the refiner with the best.  The grid arithmetic is fp32 in the order
written here (NumPy float32 scalars and arrays; the library is built without contraction), every score is an integer sum, so
the kernels must repeat this model bit for bit; the ``*64`` function is the plain restatement it is itself checked against."""
import numpy as np

import loop_closure_model as LM

F = np.float32
DEFAULTS = dict(cells=128, cell_size=1.0, window=16, yaw_div=2, yaw_half=4, z_step=0.25, tolerance=4, min_agreement=0.5)
RECORD = ("found", "k", "a", "b", "A", "occ_q", "occ_e")


def angle(shift, k, sectors, yaw_div, yaw_half):
    """theta_k of a Scan Context shift: -(shift + delta_k) 2 pi / NS with delta_k = (k - Yh) / d sectors, in fp64."""
    return -(float(shift) + float(k - yaw_half) / float(yaw_div)) * (2.0 * np.pi) / float(sectors)


def tables(sectors, yaw_div, yaw_half, up="z"):
    """-> (rot (NS Y, 2) fp32 cos / sin, pose (NS Y, 4, 4) fp64), row shift * Y + k; the poses conjugated for ``up="-y"``."""
    Y = 2 * yaw_half + 1
    rot = np.zeros((sectors * Y, 2), dtype=F)
    pose = np.tile(np.eye(4), (sectors * Y, 1, 1))
    P = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]]) if up == "-y" else np.eye(3)
    for s in range(sectors):
        for k in range(Y):
            t = angle(s, k, sectors, yaw_div, yaw_half)
            c, sn = np.cos(t), np.sin(t)
            rot[s * Y + k] = c, sn
            pose[s * Y + k, :3, :3] = P.T @ np.array([[c, -sn, 0.0], [sn, c, 0.0], [0.0, 0.0, 1.0]]) @ P
    return rot, pose


def cells_of(cloud, cs, sn, cells, cell_size, z_step, z_offset, up="z", length=None):
    """-> (keep (n,) bool, i (n,), j (n,), q (n,)): the cell and the level of every row under the planar rotation (cs, sn)."""
    x, y, z = LM.permute(cloud, up)
    n = len(x)
    cs, sn, c, zs, half = F(cs), F(sn), F(cell_size), F(z_step), F(cells // 2)
    with np.errstate(all="ignore"):
        xr = cs * x - sn * y
        yr = sn * x + cs * y
        fx = np.floor(xr / c)
        fy = np.floor(yr / c)
        h = z + F(z_offset)
        keep = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        keep &= (fx >= -half) & (fx < half) & (fy >= -half) & (fy < half) & (h > 0)
        if length is not None:
            keep &= np.arange(n) < max(0, min(int(length), n))
        lev = np.floor(h / zs)
        q = np.where(lev >= 254, 255, np.where(keep, lev, 0).astype(np.int64) + 1)
        i = np.where(keep, fx, 0).astype(np.int64) + cells // 2
        j = np.where(keep, fy, 0).astype(np.int64) + cells // 2
    return keep, i, j, q


def grid(cloud, cs, sn, cells, cell_size, z_step, z_offset, up="z", length=None):
    """-> (image (G, G) uint8: the highest level of every cell, 0 where empty; occ: the non-empty cells)."""
    keep, i, j, q = cells_of(cloud, cs, sn, cells, cell_size, z_step, z_offset, up, length)
    img = np.zeros((cells, cells), dtype=np.int64)
    np.maximum.at(img, (i[keep], j[keep]), q[keep])
    return img.astype(np.uint8), int((img > 0).sum())


def grid64(cloud, theta, cells, cell_size, z_step, z_offset, up="z"):
    """The plain restatement: the cloud turned by theta in fp64, floor of the quotients."""
    c = np.asarray(cloud, dtype=np.float64)
    x, y, z = (c[:, 0], c[:, 1], c[:, 2]) if up == "z" else (c[:, 2], -c[:, 0], -c[:, 1])
    xr, yr = np.cos(theta) * x - np.sin(theta) * y, np.sin(theta) * x + np.cos(theta) * y
    i, j = np.floor(xr / cell_size).astype(np.int64) + cells // 2, np.floor(yr / cell_size).astype(np.int64) + cells // 2
    h = z + z_offset
    keep = (i >= 0) & (i < cells) & (j >= 0) & (j < cells) & (h > 0)
    q = np.minimum(np.floor(h / z_step).astype(np.int64) + 1, 255)
    img = np.zeros((cells, cells), dtype=np.int64)
    np.maximum.at(img, (i[keep], j[keep]), q[keep])
    return img.astype(np.uint8), int((img > 0).sum())


def scores(Q, E, window, tolerance):
    """Q (Y, G, G), E (G, G) uint8 -> A (Y, 2W+1, 2W+1) int32: A[k, a+W, b+W] = sum of max(0, L - |Q_k[i][j] - E[i+a][j+b]|)
    over the cells where both are non-empty and (i + a, j + b) lies inside the grid."""
    Q, E = np.asarray(Q, dtype=np.int64), np.asarray(E, dtype=np.int64)
    Y, G, W, side = Q.shape[0], E.shape[0], int(window), 2 * int(window) + 1
    A = np.zeros((Y, side, side), dtype=np.int32)
    for k in range(Y):
        ii, jj = np.nonzero(Q[k])
        q = Q[k][ii, jj]
        for a in range(-W, W + 1):
            for b in range(-W, W + 1):
                inside = (ii + a >= 0) & (ii + a < G) & (jj + b >= 0) & (jj + b < G)
                e = E[(ii + a)[inside], (jj + b)[inside]]
                A[k, a + W, b + W] = int(np.where(e > 0, np.maximum(0, tolerance - np.abs(q[inside] - e)), 0).sum())
    return A


def choose(A, occ_q, occ_e, window, tolerance, min_agreement):
    """-> dict(found, k, a, b, A, occ_q, occ_e): the largest A, the lowest candidate index on a tie; found where A > 0 and, in
    fp32, (float)A >= m (float)(L min(occ_Qk, occ_E)).  (A = 0 says nothing about the offset: two empty images, whose bound
    is 0 too, or m = 0, are no find.)"""
    W, side = int(window), 2 * int(window) + 1
    flat = A.reshape(-1)
    best = int(flat.argmax())                           # argmax: the first (lowest) index of the maximum
    k, a, b = best // (side * side), best // side % side - W, best % side - W
    least = min(int(occ_q[k]), int(occ_e))
    found = int(flat[best] > 0 and F(flat[best]) >= F(min_agreement) * F(tolerance * least))
    return dict(found=found, k=k, a=a, b=b, A=int(flat[best]), occ_q=int(occ_q[k]), occ_e=int(occ_e))


def seed(rec, shift, T0, sectors, p, up="z"):
    """T1 of one stream: [R(theta_k), t] where found, t = (a c, b c, 0) in the descriptor's axes ((-b c, 0, a c) in KITTI's
    camera frame), c the fp32 cell size; T0, unchanged, where not."""
    if not rec["found"]:
        return np.array(T0, dtype=np.float64)
    Y = 2 * p["yaw_half"] + 1
    T = tables(sectors, p["yaw_div"], p["yaw_half"], up)[1][shift * Y + rec["k"]].copy()
    c = np.float64(F(p["cell_size"]))
    a, b = rec["a"], rec["b"]
    T[:3, 3] = (np.float64(a) * c, np.float64(b) * c, 0.0) if up == "z" else (np.float64(-b) * c, 0.0, np.float64(a) * c)
    return T


def search(stored, query, shift, sectors, p, z_offset=2.0, up="z", length=None, T0=None):
    """The whole step of one stream whose Scan Context match holds -> dict(E, occ_e, Q (Y, G, G), occ_q (Y,), A, record, T1).
    ``p``: the translation parameters (``DEFAULTS``); ``length`` counts for the query alone, the stored cloud is imaged whole."""
    p = dict(DEFAULTS, **p)
    Y = 2 * p["yaw_half"] + 1
    rot = tables(sectors, p["yaw_div"], p["yaw_half"], up)[0]
    args = (p["cells"], p["cell_size"], p["z_step"], z_offset, up)
    E, occ_e = grid(stored, F(1), F(0), *args)
    imgs = [grid(query, rot[shift * Y + k, 0], rot[shift * Y + k, 1], *args, length=length) for k in range(Y)]
    Q, occ_q = np.stack([g[0] for g in imgs]), np.array([g[1] for g in imgs], dtype=np.int32)
    A = scores(Q, E, p["window"], p["tolerance"])
    rec = choose(A, occ_q, occ_e, p["window"], p["tolerance"], p["min_agreement"])
    T0 = LM.start_pose(shift, sectors, up) if T0 is None else T0
    return dict(E=E, occ_e=occ_e, Q=Q, occ_q=occ_q, A=A, record=rec, T1=seed(rec, shift, T0, sectors, p, up))
