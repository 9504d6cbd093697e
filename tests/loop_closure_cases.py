"""Inputs of the loop-detector tests, shared by the CPU and the GPU files: clouds at cell centres,
the edge rows of the descriptor, random places for the search, and the revisit scene of the whole chain."""
import numpy as np

import loop_closure_model as M

F = np.float32
SHAPES = [(20, 60), (1, 8), (64, 64)]                 # (rings, sectors): the defaults, the smallest, the largest
MAX_RANGE, Z_OFFSET = 80.0, 2.0


def cell_centres(seed, rings, sectors, fill=0.6, max_range=MAX_RANGE):
    """(m, 3) fp64: one point at the centre of a random ``fill`` of the cells, heights in (-1.5, 3)."""
    rng = np.random.default_rng(seed)
    r, s = np.nonzero(rng.random((rings, sectors)) < fill)
    rad = (r + 0.5) * max_range / rings
    ang = (s + 0.5) * 2 * np.pi / sectors
    return np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-1.5, 3.0, len(r))], axis=1)


def turn(cloud, k, sectors):
    """The cloud as a sensor sees it whose landmarks lie k sectors further round: Rz(k 2 pi / NS) p."""
    a = k * 2 * np.pi / sectors
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    return cloud @ R.T


def to_camera(cloud):
    """Rows (x, y, z) with z up -> KITTI's camera frame: (x, y, z) = (z_cam, -x_cam, -y_cam)."""
    c = np.asarray(cloud)
    return np.stack([-c[:, 1], -c[:, 2], c[:, 0]], axis=1)


def pad(cloud, n, seed=0):
    """(n, 3) fp32: the rows, then repeats of random rows of them (a repeat changes no maximum)."""
    c = np.asarray(cloud, dtype=F)
    if len(c) >= n:
        return c[:n].copy()
    rng = np.random.default_rng(seed)
    return np.concatenate([c, c[rng.integers(0, len(c), n - len(c))]], axis=0)


def random_cloud(seed, n, max_range=MAX_RANGE):
    """(n, 3) fp32: radii beyond max_range, heights below the ground and a few bad rows included."""
    rng = np.random.default_rng(seed)
    rad = rng.uniform(0.0, 1.15 * max_range, n)
    ang = rng.uniform(-np.pi, np.pi, n)
    c = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-3.0, 4.0, n)], axis=1).astype(F)
    return c


def edge_rows(rings, sectors, max_range=MAX_RANGE, z_offset=Z_OFFSET):
    """(m, 3) fp32 rows on every edge of the bin arithmetic; each row's height is its own, so a wrong bin shows."""
    ring_b, dx, dy = M.tables(rings, sectors, max_range)
    rows = []
    up, down = lambda v: np.nextafter(F(v), F(np.inf)), lambda v: np.nextafter(F(v), F(-np.inf))
    for k in sorted({0, rings // 2, rings - 1}):      # r2 exactly b_k (the roots are exact in fp32 for the tested shapes)
        root = F(np.sqrt(np.float64(ring_b[k])))
        for x in (down(down(root)), down(root), root, up(root), up(up(root))):
            rows.append((x, 0.0, 0.5))
            rows.append((0.0, -x, 0.25))
    for s in sorted({0, 1, sectors // 4, sectors // 2, sectors - 1}):
        for t in (1.0, 7.3, 0.6 * max_range):
            x, y = F(t) * dx[s], F(t) * dy[s]
            for xx in (down(x), x, up(x)):
                for yy in (down(y), y, up(y)):
                    rows.append((xx, yy, 1.0))
    rows += [(0.0, 0.0, 1.0), (np.nan, 1.0, 1.0), (1.0, np.inf, 1.0), (1.0, 1.0, -np.inf), (-np.inf, 1.0, 1.0),
             (3.0, 1.0, np.nan)]
    bumped = len(rows)
    # h = 0, one ulp to each side of it, and (where z_offset is 0) the smallest positive float
    rows += [(5.0, 2.0, -z_offset), (5.0, -2.0, up(F(-z_offset))), (-5.0, 2.0, down(F(-z_offset))),
             (-5.0, -2.0, F(-z_offset) + np.nextafter(F(0), F(1)))]
    rows += [(11.0, 3.0, 0.1), (11.01, 3.01, 0.7), (11.02, 2.99, 0.3)]          # one cell (at the default shape), three heights
    out = np.array(rows, dtype=F)
    bump = (np.arange(bumped) % 7).astype(F) * F(0.125)
    out[:bumped, 2] = np.where(np.isfinite(out[:bumped, 2]), out[:bumped, 2] + bump, out[:bumped, 2])
    return out


def places(seed, count, rings, sectors, n=192, max_range=MAX_RANGE):
    """``count`` random places as the model describes them: (Dn (count, NR, NS), masks, clouds (count, n, 3))."""
    clouds = [pad(cell_centres(seed * 1000 + e, rings, sectors, fill=0.35, max_range=max_range), n, seed=e) for e in range(count)]
    desc = [M.descriptor(c, rings, sectors, max_range, Z_OFFSET) for c in clouds]
    return np.stack([d[1] for d in desc]), [d[2] for d in desc], np.stack(clouds)


def margins(Qn, qmask, En, emask):
    """fp64 runner-up margins of a query against places: (entry margin, shift margin of the winner, the fp32 model's own
    error against fp64)."""
    d64 = M.distances64(Qn, qmask, En, emask)
    d32 = M.distances(Qn, qmask, En, emask)
    fin = np.isfinite(d64)
    err = float(np.abs(d32[fin].astype(np.float64) - d64[fin]).max()) if fin.any() else 0.0
    best = d64.min(axis=1)
    e = int(best.argmin())
    entry = float(np.partition(best, 1)[1] - best[e]) if len(best) > 1 else np.inf
    row = np.sort(d64[e])
    return entry, float(row[1] - row[0]), err


# ---- the revisit scene of the whole chain ------------------------------------------------------------------------------

def scene(seed, half=18.0, half_y=None, centre=(0.0, 0.0)):
    """Walls and boxes, asymmetric: sampled by ``world_points``.  A room of 2 half x 2 half_y (a square turned by 90 degrees
    looks like itself to a polar descriptor: ``half_y`` breaks that, a ``centre`` off the sensor's path the half turn) with a floor, an inner wall and boxes of different
    heights, so that yaw and position are observable."""
    rng = np.random.default_rng(seed)
    half_y = half if half_y is None else half_y
    boxes = [(rng.uniform(-half + 2, half - 2), rng.uniform(-half_y + 2, half_y - 2), rng.uniform(0.8, 2.5),
              rng.uniform(0.8, 2.5), rng.uniform(0.5, 3.0)) for _ in range(9)]
    return dict(half=half, half_y=half_y, centre=centre, boxes=boxes, wall=(rng.uniform(-6, 6), rng.uniform(2, 8)),
                heights=rng.uniform(2.0, 4.0, 4))


def world_points(sc, m, seed):
    """(m, 3) fp64 points on the scene's surfaces, world frame, the ground at z = -1.7 (a sensor 1.7 m up)."""
    rng = np.random.default_rng(seed)
    half, g = (sc["half"], sc["half_y"]), -1.7
    parts = []
    k = m // 4
    parts.append(np.stack([rng.uniform(-half[0], half[0], k), rng.uniform(-half[1], half[1], k), np.full(k, g)], axis=1))  # floor
    per = m // 8
    for i, (axis, sign) in enumerate(((0, 1), (0, -1), (1, 1), (1, -1))):                                        # outer walls
        u, z = rng.uniform(-half[1 - axis], half[1 - axis], per), g + rng.uniform(0, sc["heights"][i], per)
        p = np.zeros((per, 3))
        p[:, axis], p[:, 1 - axis], p[:, 2] = sign * half[axis], u, z
        parts.append(p)
    wx, wl = sc["wall"]
    u = rng.uniform(0, wl, per)
    parts.append(np.stack([np.full(per, wx), u - 2.0, g + rng.uniform(0, 2.5, per)], axis=1))                      # inner wall
    rest = m - sum(len(p) for p in parts)
    per_box = rest // len(sc["boxes"])
    for bi, (cx, cy, sx, sy, h) in enumerate(sc["boxes"]):
        cnt = per_box if bi < len(sc["boxes"]) - 1 else rest - per_box * (len(sc["boxes"]) - 1)
        face = rng.integers(0, 5, cnt)
        a, b = rng.uniform(-1, 1, cnt), rng.uniform(0, 1, cnt)
        p = np.zeros((cnt, 3))
        p[:, 0] = np.where(face == 0, cx - sx, np.where(face == 1, cx + sx, cx + a * sx))
        p[:, 1] = np.where(face == 2, cy - sy, np.where(face == 3, cy + sy, np.where(face < 2, cy + a * sy, cy + (2 * b - 1) * sy)))
        p[:, 2] = np.where(face == 4, g + h, g + b * h)
        parts.append(p)
    return np.concatenate(parts, axis=0)[:m] + np.array([sc["centre"][0], sc["centre"][1], 0.0])


def pose(x, y, yaw):
    T = np.eye(4)
    T[:3, :3] = [[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]]
    T[:2, 3] = x, y
    return T


def scan(points, T, n, seed):
    """(n, 3) fp32: a fresh subset of the world points in the sensor frame of pose T (world <- sensor), shuffled."""
    rng = np.random.default_rng(seed)
    idx = rng.permutation(len(points))[:n]
    p = points[idx]
    return ((p - T[:3, 3]) @ T[:3, :3]).astype(F)


def closed_path(frames=40, radius=6.0, yaw_offset=np.pi / 2, shift=0.3):
    """Poses of a sensor on a circle that comes back to its start ``shift`` metres off and turned by ``yaw_offset``."""
    out = []
    for k in range(frames):
        a = 2 * np.pi * k / (frames - 1)
        last = k == frames - 1
        out.append(pose(radius * np.cos(a) - radius + (shift if last else 0.0), radius * np.sin(a),
                        a + np.pi / 2 + (yaw_offset - 2 * np.pi if last else 0.0) if k else np.pi / 2))
    return out


REVISIT_N, REVISIT_MIN_ID = 1024, 20
REVISIT_MAX_DISTANCE = 2.0      # the verifying refiner's max_dist: translation is not searched, so a place further off than
#                                 the pairing radius cannot be closed and is not a candidate


def revisit():
    """The whole-chain case -> dict(path, frames (K, 2, n, 3) fp32, chain (K, 4, 4), positions (K, 3)).  Stream 0 drives the
    closed path through a rectangular room whose centre lies off the path (no turn of the room looks like the room); stream 1
    sees the same frames but ends, at the same pose index, in a different place.  ``chain``: the true relative poses with a
    fixed-seed drift, what an odometry would hand the pose graph; ``positions``: the translations of their products, what
    the distance gate reads."""
    if not _REVISIT:
        pts = world_points(scene(3, half=10.0, half_y=6.0, centre=(2.0, 1.5)), 20000, 4)
        other = world_points(scene(11, half=7.0), 20000, 12)
        path = closed_path(radius=3.0)
        home = [scan(pts, T, REVISIT_N, 100 + k) for k, T in enumerate(path)]
        away = home[:-1] + [scan(other, path[-1], REVISIT_N, 999)]
        rng = np.random.default_rng(5)
        chain, X = [np.eye(4)], [np.eye(4)]
        for k in range(1, len(path)):
            a = rng.normal(size=3)
            a, ang = a / np.linalg.norm(a), rng.normal() * 0.004
            Kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
            drift = np.eye(4)
            drift[:3, :3] = np.eye(3) + np.sin(ang) * Kx + (1.0 - np.cos(ang)) * (Kx @ Kx)
            drift[:3, 3] = rng.normal(size=3) * 0.02
            chain.append((np.linalg.inv(path[k - 1]) @ path[k]) @ drift)
            X.append(X[-1] @ chain[-1])
        _REVISIT.update(path=path, frames=np.stack([np.stack(home), np.stack(away)], axis=1), chain=np.stack(chain),
                        positions=np.stack(X)[:, :3, 3])
    return _REVISIT


_REVISIT = {}


# ---- search cases: decided by the model on the CPU, repeated by the kernels on the GPU ------------------------------------

SEARCH_COUNTS = (1, 63, 64, 65, 257)
SEARCH_SHAPE = (20, 60)
SEARCH_N = 192
MIN_ID = 10


def search_case(count, shift=7):
    """``count`` places with frame ids 3 e, and a query that is place count // 2 seen ``shift`` sectors further round with a
    twelfth of its points gone: the winner and its shift are known, and every other place is a runner-up."""
    rings, sectors = SEARCH_SHAPE
    Dn, masks, clouds = places(count, count, rings, sectors, SEARCH_N)
    want = count // 2
    src = cell_centres(count * 1000 + want, rings, sectors, fill=0.35)
    query = pad(turn(src[np.arange(len(src)) % 12 != 0], shift, sectors), SEARCH_N, seed=99)
    return dict(count=count, Dn=Dn, masks=masks, clouds=clouds, frame_ids=np.arange(count, dtype=np.int32) * 3, query=query,
                f=3 * count + 50, want=want, shift=shift)
