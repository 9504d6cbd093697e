"""The global map's rule in NumPy: what ``csrc/global_map.hip`` must reproduce bit for bit.

Row i < length[k] of keyframe k has the global row id g = k n + i, the world point w = float32(X[frame[k]] p) (fp64,
((m0 x + m1 y) + m2 z) + m3 per axis, one rounding) and the key of section 19 applied to w.  A row is no candidate where w
is not finite, |w_a / v| >= 2^31 on an axis, or its keyframe's frame id has no pose.  The map is the w of the lowest g of
every key, in ascending g."""
import numpy as np

F = np.float32
MASK = (1 << 64) - 1
EMPTY = np.uint64(MASK)
K0, K1, K2 = 73856093, 19349669, 83492791


def world(cloud, T):
    """cloud (n, 3) fp32, T (4, 4) fp64 -> (n, 3) fp32."""
    p = np.asarray(cloud, dtype=F).astype(np.float64)
    T = np.asarray(T, dtype=np.float64)
    with np.errstate(all="ignore"):
        w = ((T[None, :3, 0] * p[:, 0:1] + T[None, :3, 1] * p[:, 1:2]) + T[None, :3, 2] * p[:, 2:3]) + T[None, :3, 3]
        return w.astype(F)


def keys(w, v):
    """w (m, 3) fp32 -> (candidate (m,) bool, h (m,) uint64)."""
    with np.errstate(all="ignore"):
        d = w.astype(np.float64) / np.float64(v)
        inside = np.abs(d) < 2147483648.0                        # False for NaN and for +-inf
        q = np.rint(np.where(inside, d, 0.0)).astype(np.int64).astype(np.uint64)
        h = np.uint64(K0) * q[:, 0] + np.uint64(K1) * q[:, 1] + np.uint64(K2) * q[:, 2]
    return inside.all(axis=1), h


def rows(clouds, frames, lengths, X, v):
    """Every row of the bank in g order -> (w (K n, 3), candidate (K n,), h (K n,), source (K n, 2))."""
    clouds = np.asarray(clouds, dtype=F)
    K, n = clouds.shape[:2]
    X = np.asarray(X, dtype=np.float64)
    w = np.zeros((K, n, 3), dtype=F)
    cand = np.zeros((K, n), dtype=bool)
    h = np.zeros((K, n), dtype=np.uint64)
    src = np.zeros((K, n, 2), dtype=np.int32)
    for k in range(K):
        f = int(frames[k])
        src[k, :, 0], src[k, :, 1] = f, np.arange(n)
        if not 0 <= f < len(X):
            continue
        w[k] = world(clouds[k], X[f])
        c, h[k] = keys(w[k], v)
        cand[k] = c & (np.arange(n) < min(max(int(lengths[k]), 0), n))
    return w.reshape(-1, 3), cand.reshape(-1), h.reshape(-1), src.reshape(-1, 2)


def build(clouds, X, v, frames=None, lengths=None, capacity=None):
    """clouds (K, n, 3) fp32; X (frames, 4, 4) fp64 read by ``frames`` (K,) (None: keyframe k at X[k]); lengths (K,) or None
    -> (points (m, 3) fp32, source (m, 2) int32 = (frame id, row), total), m = min(total, capacity)."""
    clouds = np.asarray(clouds, dtype=F)
    K, n = clouds.shape[:2]
    frames = np.arange(K) if frames is None else np.asarray(frames)
    lengths = np.full(K, n) if lengths is None else np.asarray(lengths)
    if K == 0:
        return np.zeros((0, 3), dtype=F), np.zeros((0, 2), dtype=np.int32), 0
    w, cand, h, src = rows(clouds, frames, lengths, X, v)
    g = np.flatnonzero(cand)                                     # ascending g
    _, first = np.unique(h[g], return_index=True)                # the first occurrence = the lowest g of every key
    win = g[np.sort(first)]
    total = len(win)
    if capacity is not None:
        win = win[:capacity]
    return w[win], src[win], total


class Bank:
    """One stream of ``GlobalMap`` on the host: the bank, and how many of its keyframes the map holds."""

    def __init__(self, n, max_keyframes, stride=1, max_new=1):
        self.n, self.MK, self.stride, self.max_new = n, max_keyframes, stride, max_new
        self.reset()
        self.overflow = False

    def reset(self):
        self.clouds, self.frames, self.lengths, self.built = [], [], [], 0

    def advance(self, cloud, frame_id, length=None, restart=False):
        if restart:
            self.reset()
        if frame_id >= 0 and frame_id % self.stride == 0:
            if len(self.frames) < self.MK:
                self.clouds.append(np.array(cloud, dtype=F))
                self.frames.append(int(frame_id))
                self.lengths.append(self.n if length is None else min(max(int(length), 0), self.n))
            else:
                self.overflow = True
        self.built += min(len(self.frames) - self.built, self.max_new)

    def rebuild(self):
        self.built = len(self.frames)

    def invalidate(self):
        self.built = 0

    def map(self, X, v, capacity=None):
        """The map of the keyframes [0, built) at X (frames, 4, 4)."""
        b = self.built
        if b == 0:
            return np.zeros((0, 3), dtype=F), np.zeros((0, 2), dtype=np.int32), 0
        return build(np.stack(self.clouds[:b]), X, v, self.frames[:b], self.lengths[:b], capacity)
