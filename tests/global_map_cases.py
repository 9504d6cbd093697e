"""Inputs of the global map's tests, decided on the CPU by ``global_map_model`` and repeated by the
kernels on the GPU: every family of the rule's edges as ``(clouds (K, n, 3) fp32, poses (K, 4, 4) fp64, lengths or None)``."""
import numpy as np

import global_map_model as model

F = np.float32
NS = (1, 63, 64, 65, 255, 256, 257, 1024)                # one row; around a wave; around a workgroup; several workgroups
KS = (1, 2, 3, 40)
VOXELS = (0.1, 0.3, 0.5)
MARKER_VOXEL = (1355969, -5175622, 0)                    # its hash is the table's empty marker


def pose(rng, spread=2.0, angle=0.5):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    th = rng.normal() * angle
    Kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)
    T[:3, 3] = rng.normal(size=3) * spread
    return T


def poses(seed, K, **kw):
    rng = np.random.default_rng([seed, 77])
    return np.stack([pose(rng, **kw) for _ in range(K)])


def identity(K):
    return np.tile(np.eye(4), (K, 1, 1))


def uniform(seed, K, n, v):
    """Rows spread so that most voxels hold one row and keyframes overlap."""
    rng = np.random.default_rng([seed, K, n])
    side = v * max(2.0, (K * n) ** (1.0 / 3.0))
    return rng.uniform(-side, side, (K, n, 3)).astype(F), poses(seed, K, spread=0.5 * side), None


def dense(seed, K, n, v):
    """About eight rows per voxel."""
    rng = np.random.default_rng([seed, K, n, 8])
    side = 0.5 * v * max(1.0, (K * n / 8.0) ** (1.0 / 3.0))
    return rng.uniform(-side, side, (K, n, 3)).astype(F), poses(seed, K, spread=0.1 * side, angle=0.02), None


def one_voxel(seed, K, n, v):
    rng = np.random.default_rng([seed, K, n, 1])
    return (rng.uniform(-0.2 * v, 0.2 * v, (K, n, 3)) + 3.0 * v).astype(F), identity(K), None


def same_cloud(seed, K, n, v):
    """Every keyframe the same cloud at the identity: only keyframe 0 wins."""
    c, _, _ = uniform(seed, 1, n, v)
    return np.repeat(c, K, axis=0), identity(K), None


def shifted(seed, K, n, v):
    """The same cloud at poses that differ by less than a voxel (even k) and by more (odd k)."""
    c, _, _ = uniform(seed, 1, n, v)
    X = identity(K)
    for k in range(K):
        X[k, :3, 3] = (0.07 * v * k, -0.05 * v * k, 0.0) if k % 2 == 0 else (2.3 * v * k, 1.7 * v * k, -3.1 * v)
    return np.repeat(c, K, axis=0), X, None


def halfway(seed, K, n, v):
    """World points (j + 1/2) v on every axis (exact at v = 0.5) reached through a translation."""
    rng = np.random.default_rng([seed, K, n, 2])
    t = np.array([0.25, -0.75, 1.25])
    X = identity(K)
    X[:, :3, 3] = t
    j = rng.integers(-6, 6, (K, n, 3)).astype(np.float64)
    w = (j + 0.5) * v
    return (w - t).astype(F), X, None


def non_finite(seed, K, n, v):
    c, X, _ = uniform(seed, K, n, v)
    rng = np.random.default_rng([seed, 3])
    bad = rng.random((K, n)) < 0.3
    bad[0, 0] = True
    vals = np.array([np.nan, np.inf, -np.inf], dtype=F)
    c[bad, rng.integers(0, 3, bad.sum())] = vals[rng.integers(0, 3, bad.sum())]
    return c, X, None


def far_pose(seed, K, n, v):
    """The last keyframe's translation pushes |w / v| past 2^31 on one axis; with K = 1 that is the only keyframe."""
    c, X, _ = uniform(seed, K, n, v)
    X[-1, 1, 3] = 2.2e9 * v
    if K > 2:
        X[1, 0, 3] = -(2.0 ** 31) * v                    # exactly the bound for a row at x = 0
        c[1, 0] = 0.0
    return c, X, None


def bad_pose(seed, K, n, v):
    c, X, _ = uniform(seed, K, n, v)
    X[-1, 0, 1] = np.nan
    if K > 1:
        X[0, 2, 3] = np.inf
    return c, X, None


def marker(seed, K, n, v):
    """Rows in the voxel whose hash is the empty marker, at the identity, among ordinary rows, in several keyframes."""
    c, _, _ = uniform(seed, K, n, v)
    centre = np.array(MARKER_VOXEL, dtype=np.float64) * v
    for k in range(K):
        c[k, n // 2] = centre
        c[k, -1] = centre
    ok, h = model.keys(c[0, -1:].copy(), v)
    assert ok[0] and h[0] == model.EMPTY, (v, h)
    return c, identity(K), None


def partial(seed, K, n, v):
    c, X, _ = dense(seed, K, n, v)
    rng = np.random.default_rng([seed, 4])
    lengths = rng.integers(0, n + 1, K)
    lengths[0] = n // 2
    if K > 1:
        lengths[1] = 0
    if K > 2:
        lengths[2] = n
    return c, X, lengths.astype(np.int32)


FAMILIES = dict(uniform=uniform, dense=dense, one_voxel=one_voxel, same_cloud=same_cloud, shifted=shifted, halfway=halfway,
                non_finite=non_finite, far_pose=far_pose, bad_pose=bad_pose, marker=marker, partial=partial)

# Every family at every voxel size on shapes that cross a wave, a workgroup and a keyframe; every (n, K) on two families.
TABLE = [(name, n, K, v) for name in FAMILIES for v in VOXELS for n, K in ((65, 3), (257, 2))] + \
        [(name, n, K, 0.3) for name in ("uniform", "dense") for n in NS for K in KS]
SMALL = [(name, n, K, v) for name in FAMILIES for v in VOXELS for n, K in ((65, 3),)]     # for the row-by-row second model


def case(name, n, K, v, seed=1):
    return FAMILIES[name](seed, K, n, v)


def schedule(S=3, n=96, calls=12, seed=5):
    """A stateful schedule for S = 3 streams: per call (clouds (S, n, 3), frame_ids (S,), active (S,), restart (S,), lengths
    (S,)).  Stream 1 idles in some calls, stream 2 restarts in mid-sequence; frame ids count the stream's own frames."""
    rng = np.random.default_rng(seed)
    ids = np.zeros(S, dtype=np.int64)
    out = []
    for c in range(calls):
        active = np.ones(S, dtype=np.int32)
        restart = np.zeros(S, dtype=np.int32)
        if c in (2, 3, 7):
            active[1] = 0
        if c == 6:
            restart[2] = 1
            ids[2] = 0
        clouds = rng.uniform(-1.5, 1.5, (S, n, 3)).astype(F)
        lengths = np.where(rng.random(S) < 0.3, rng.integers(0, n + 1, S), n).astype(np.int32)
        out.append((clouds, ids.astype(np.int32).copy(), active, restart, lengths))
        ids += active
    return out


def trajectory(S, frames, seed=9):
    """(frames, S, 4, 4) fp64: smooth paths with steps of about a voxel."""
    rng = np.random.default_rng(seed)
    X = np.zeros((frames, S, 4, 4))
    for s in range(S):
        T = np.eye(4)
        for f in range(frames):
            X[f, s] = T
            T = T @ pose(rng, spread=0.2, angle=0.05)
    return X
