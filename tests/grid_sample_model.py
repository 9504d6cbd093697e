"""NumPy model of voxel grid sampling (``preprocess.grid_sample``), written from the rule alone:

    q_a = rint(double(p_a) / v)        fp64 division, round half to even
    h   = 73856093 q_x + 19349669 q_y + 83492791 q_z    int64 with wraparound
    winner = the lowest-index candidate row of its cloud with that h

A row with a non-finite coordinate or |p_a / v| >= 2^31 on an axis is no candidate; neither is a row at or past ``length``
or with ``keep == 0``.  The winners come back in ascending row order."""
import numpy as np

PRIMES = (73856093, 19349669, 83492791)
EMPTY_KEY = -1                      # the bit pattern (all ones) the kernel's table uses for an empty slot


def voxel_hash(points, voxel):
    """points (n, >=3) float32 -> (h (n,) int64, ok (n,) bool: the row may be a candidate)."""
    p = np.asarray(points)
    assert p.dtype == np.float32 and p.ndim == 2 and p.shape[1] >= 3
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        d = p[:, :3].astype(np.float64) / np.float64(voxel)
        ok = (np.isfinite(p[:, :3]) & (np.abs(d) < 2.0 ** 31)).all(axis=1)
        q = np.rint(np.where(ok[:, None], d, 0.0)).astype(np.int64)
        h = np.int64(PRIMES[0]) * q[:, 0] + np.int64(PRIMES[1]) * q[:, 1] + np.int64(PRIMES[2]) * q[:, 2]
    return h, ok


def grid_keep(points, voxel, length=None, keep=None):
    """One cloud -> keep mask (n,) int32 with 1 at the winners."""
    n = points.shape[0]
    h, cand = voxel_hash(points, voxel)
    if length is not None:
        cand &= np.arange(n) < length
    if keep is not None:
        cand &= np.asarray(keep) != 0
    rows = np.flatnonzero(cand)
    out = np.zeros(n, dtype=np.int32)
    if rows.size:
        first = np.unique(h[rows], return_index=True)[1]        # the first occurrence of every hash among the candidates
        out[rows[first]] = 1
    return out


def grid_keep_batch(points, voxel, lengths=None, keep=None):
    """points (b, n, 3|4) -> (keep (b, n) int32, counts (b,) int32)."""
    masks = np.stack([grid_keep(points[c], voxel, None if lengths is None else int(lengths[c]),
                                None if keep is None else keep[c]) for c in range(points.shape[0])])
    return masks, masks.sum(axis=1).astype(np.int32)


def solve_hash(target, bound=1 << 24):
    """Integers (qx, qy, qz), each |q| <= bound, with PRIMES . q == target exactly (no wraparound needed), or None.
    For each small qz the congruence a qx = target - c qz (mod b) fixes qx modulo b; qy follows by exact division."""
    a, b, c = PRIMES
    inv_a = pow(a, -1, b)
    for qz in range(0, 4000):
        for z in (qz, -qz):
            rhs = target - c * z
            qx = (rhs * inv_a) % b
            if qx > b // 2:
                qx -= b
            rest = rhs - a * qx
            assert rest % b == 0
            qy = rest // b
            if max(abs(qx), abs(qy), abs(z)) <= bound:
                return qx, qy, z
    return None
