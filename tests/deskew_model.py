"""NumPy model (fp64) of the motion compensation of raw sweeps, the rule the device kernels follow:

1. candidates are the rows the filter keeps (``keep``), below ``length``;
2. tau_min / tau_max over the candidates with a finite time; alpha_i = (tau_i - tau_min) / (tau_max - tau_min), 0 for every
   row without a time range and for a candidate whose own time is not finite;
3. the motion is a pose row [tx ty tz qw qx qy qz]: |q|^2 < 1e-8 is the identity rotation, otherwise the unit quaternion
   with w >= 0, theta = 2 atan2(|v|, w), axis k = v / |v|; R(alpha) is the rotation by alpha * theta about k;
4. p'_i = R(alpha_i) p_i + alpha_i t in fp64, rounded to fp32 once;
5. rows with alpha_i = 0, rows that are no candidates, and every row under the identity motion keep their bits.
"""
import numpy as np

IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float32)


def _row(angle_deg, axis, t, scale=1.0):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    half = np.deg2rad(angle_deg) / 2
    q = scale * np.concatenate([[np.cos(half)], np.sin(half) * axis])
    return np.concatenate([np.asarray(t, dtype=np.float64), q]).astype(np.float32)


# The motions every test runs: the angles of the issue, a quaternion with w < 0, a non-unit one, and |q|^2 < 1e-8.
MOTIONS = {
    "0deg": _row(0.0, [0, 0, 1], [0.8, 0.1, -0.05]),
    "1e-9deg": _row(1e-9, [0.3, -0.2, 0.9], [1.1, -0.2, 0.03]),
    "2deg": _row(2.0, [0.05, 0.02, 1.0], [1.3, 0.04, -0.02]),
    "90deg": _row(90.0, [1, 2, -3], [0.5, 0.5, 0.5]),
    "179deg": _row(179.0, [-0.4, 0.1, 0.7], [-2.0, 0.3, 0.1]),
    "w<0": _row(-40.0, [0.2, 0.9, 0.1], [0.9, 0.0, 0.2], scale=-1.0),
    "non-unit": _row(30.0, [0, 1, 0.5], [0.2, -1.4, 0.6], scale=2.5),
    "nq<1e-8": np.array([0.7, -0.3, 0.2, 1e-5, 2e-5, 0, 0], dtype=np.float32),
}
assert MOTIONS["w<0"][3] < 0 and float((MOTIONS["nq<1e-8"][3:].astype(np.float64) ** 2).sum()) < 1e-8


def quat2mat(q):
    """The reference's quat2mat (the nibabel form: valid for non-unit quaternions, the identity below 1e-8), fp64."""
    w, x, y, z = np.asarray(q, dtype=np.float64)
    nq = w * w + x * x + y * y + z * z
    if nq < 1e-8:
        return np.eye(3)
    s = 2.0 / nq
    X, Y, Z = x * s, y * s, z * s
    wX, wY, wZ, xX, xY, xZ, yY, yZ, zZ = w * X, w * Y, w * Z, x * X, x * Y, x * Z, y * Y, y * Z, z * Z
    return np.array([[1.0 - (yY + zZ), xY - wZ, xZ + wY], [xY + wZ, 1.0 - (xX + zZ), yZ - wX],
                     [xZ - wY, yZ + wX, 1.0 - (xX + yY)]])


def axis_angle(row):
    """A pose row -> (unit axis k (3,), theta in [0, pi], t (3,)), all fp64 (rule 3)."""
    row = np.asarray(row, dtype=np.float32).astype(np.float64)
    t, q = row[:3], row[3:]
    nq = float((q * q).sum())
    k, theta = np.array([1.0, 0.0, 0.0]), 0.0
    if not nq < 1e-8:
        q = q / np.sqrt(nq)
        if q[0] < 0:
            q = -q
        nv = float(np.sqrt((q[1:] * q[1:]).sum()))
        theta = 2.0 * np.arctan2(nv, q[0])
        if nv > 0:
            k = q[1:] / nv
    return k, theta, t


def alphas(times, keep=None, length=None):
    """(n,) times -> (alpha (n,) fp64, candidate mask (n,) bool) (rules 1 and 2)."""
    tau = np.asarray(times).astype(np.float64)
    n = tau.shape[0]
    cand = np.ones(n, dtype=bool) if keep is None else np.asarray(keep) != 0
    cand = cand & (np.arange(n) < (n if length is None else length))
    use = cand & np.isfinite(tau)
    alpha = np.zeros(n, dtype=np.float64)
    if use.any():
        lo, hi = tau[use].min(), tau[use].max()
        if hi > lo:
            with np.errstate(over="ignore", invalid="ignore"):
                alpha[use] = (tau[use] - lo) / (hi - lo)
    return alpha, cand


def deskew(points, times, row, keep=None, length=None):
    """points (n, >=3) fp32, times (n,), row (7,) -> (m (n, 3) fp64: the model's value before the last rounding, out (n, 3)
    fp32: m rounded once, with the bits of ``points`` wherever rule 5 says so)."""
    p32 = np.ascontiguousarray(np.asarray(points, dtype=np.float32)[:, :3])
    p = p32.astype(np.float64)
    alpha, _ = alphas(times, keep, length)
    k, theta, t = axis_angle(row)
    phi = alpha * theta
    s, c = np.sin(phi)[:, None], np.cos(phi)[:, None]
    with np.errstate(invalid="ignore"):                    # non-finite coordinates stay what they are
        m = p * c + np.cross(k[None], p) * s + k[None] * ((p @ k)[:, None] * (1.0 - c)) + alpha[:, None] * t[None]
    same = (alpha == 0.0) | (theta == 0.0 and not t.any())
    m[same] = p[same]
    out = m.astype(np.float32)
    out[same] = p32[same]
    return m, out


def deskew_batch(points, times, rows, keep=None, lengths=None):
    """(b, n, c), (b, n), (b, 7) -> (m (b, n, 3) fp64, out (b, n, 3) fp32)."""
    res = [deskew(points[c], times[c], rows[c], None if keep is None else keep[c], None if lengths is None else lengths[c])
           for c in range(points.shape[0])]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def ulp32(m):
    """The spacing of fp32 at the fp64 values m (the binade of |m|; the subnormal spacing below 2^-126)."""
    m = np.abs(np.asarray(m, dtype=np.float64))
    _, e = np.frexp(m)
    return np.ldexp(1.0, np.where(m == 0.0, -149, np.maximum(e - 24, -149)))


def bound(m, points, row):
    """|out - m| <= 1/2 ulp32(m) + 1e-12 (|p| + |t|): correct rounding of a value within fp64 noise of the model."""
    p = np.asarray(points, dtype=np.float32)[..., :3].astype(np.float64)
    t = np.asarray(row, dtype=np.float32)[..., :3].astype(np.float64)
    scale = np.linalg.norm(p, axis=-1) + np.linalg.norm(t, axis=-1)[..., None]
    return 0.5 * ulp32(m) + 1e-12 * scale[..., None]
