"""Edge cases of the projective registration (csrc/projective.hip), built in NumPy alone: every case is
a dict with the ``edge`` it is about and the inputs of one op.  tests/test_projective_cases_cpu.py proves on the model
(tests/projective_model.py) that each case reaches its edge and tells the model from the planted fault that the edge is
about; tests/test_gpu_projective_edges.py runs the same cases through the kernels.

Two devices make an edge decidable although the last bit of an fp32 atan2 / asin is not promised: exact arguments (points
on the axes, where both functions return 0, +-pi/2 or +-pi, in an image with a symmetric field of view) and planted images
(model_build, accumulate and map_push take images, so any value can stand at any pixel; short mantissas keep sums and
differences exact).  Every other point is kept >= BAND px (fp64) from a rounding boundary."""
import functools

import numpy as np

import icp_model as icp
import projective_model as model

BAND = 1e-3
F = np.float32
SYM = dict(up_fov=15.0, down_fov=-15.0)          # |up| = |down|: z = 0 is row H / 2 exactly
LIDAR = dict(up_fov=3.0, down_fov=-24.8)
HALF_ULP = 2.0 ** -24                            # one fp32 rounding of a component of a unit vector


def image(H, W, fov):
    return model.image(H, W, fov["up_fov"], fov["down_fov"])


def ray(im, row, col, rng=4.0):
    """The fp32 point at the fp64 image coordinates (row, col) (arrays or scalars) and range ``rng``."""
    row, col = np.asarray(row, dtype=np.float64), np.asarray(col, dtype=np.float64)
    phi = (1.0 - row / im["H"]) * im["fov64"] - im["down64"]
    theta = (2.0 * col / im["W"] - 1.0) * np.pi
    d = np.stack([np.cos(phi) * np.cos(-theta), np.cos(phi) * np.sin(-theta), np.sin(phi)], axis=-1)
    return (d * np.asarray(rng, dtype=np.float64)[..., None]).astype(F)


def centres(im, rng=4.0):
    """(H * W, 3) fp32: one point through every pixel's centre."""
    H, W = im["H"], im["W"]
    i = np.arange(H * W)
    return ray(im, i // W, i % W, rng)


def short(p, bits=10):
    """p rounded to multiples of 2^-bits: sums with 0.5, 0.25 and 0.125 stay exact in fp32 (|p| < 16)."""
    return (np.round(np.asarray(p, dtype=np.float64) * 2.0 ** bits) / 2.0 ** bits).astype(F)


def range32(p):
    p = np.asarray(p, dtype=F)
    return np.sqrt((p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]) + p[..., 2] * p[..., 2], dtype=F)


def bits32(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)


# ---- vertex map ----------------------------------------------------------------------------------------------------------------

def _vertex(edge, H, W, fov, streams, lands=None, refused=(), wins=None, exact=(), faults=()):
    """streams: a list of dict(points (R, C), length, keep); shorter streams are padded with origin rows (no range)."""
    R = max(len(st["points"]) for st in streams)
    C = streams[0]["points"].shape[1]
    pts = np.zeros((len(streams), R, C), dtype=F)
    keep = np.ones((len(streams), R), dtype=np.int32)
    for s, st in enumerate(streams):
        pts[s, :len(st["points"])] = st["points"]
        if st.get("keep") is not None:
            keep[s, :len(st["keep"])] = st["keep"]
    has_len, has_keep = any("length" in st for st in streams), any(st.get("keep") is not None for st in streams)
    lengths = np.array([st.get("length", R) for st in streams], dtype=np.int32) if has_len or not has_keep else None
    return dict(edge=edge, H=H, W=W, fov=fov, im=image(H, W, fov), points=pts, lengths=lengths,
                keep=keep if has_keep else None, lands=lands or {}, refused=list(refused), wins=wins or {},
                exact=set(exact), faults=tuple(faults))


EXACT_SHAPES = ((5, 10), (7, 6), (1, 1))


def exact_arguments(H, W):
    """Points on the axes in a symmetric field of view: row H / 2 and columns W / 2, W / 4, 3 W / 4, 0 and W exactly."""
    pts = np.array([[2.0, 0.0, 0.0], [0.0, 3.0, 0.0], [0.0, -3.0, 0.0], [-2.5, 0.0, 0.0], [-2.0, -0.0, 0.0]], dtype=F)
    want = {(5, 10): {0: (2, 5), 1: (2, 2), 2: (2, 8), 3: (2, 0)},      # 2.5 -> 2; 2.5 -> 2, 7.5 -> 8
            (7, 6): {0: (4, 3), 1: (4, 2), 2: (4, 4), 3: (4, 0)},       # 3.5 -> 4; 1.5 -> 2, 4.5 -> 4
            (1, 1): {0: (0, 0), 1: (0, 0), 3: (0, 0)}}[(H, W)]          # 0.5 -> 0; 0.25 -> 0; 0.75 -> 1: outside
    refused = [(0, 4)] + ([(0, 2)] if (H, W) == (1, 1) else [])
    lands = {(0, i): p for i, p in want.items()}
    wins = {(0,) + p: i for i, p in want.items()} if (H, W) != (1, 1) else {(0, 0, 0): 0}
    exact = [(0, i) for i in range(5)]
    if (H, W) == (1, 1):                                                # with margin: one that lands, one outside the field
        im = image(H, W, SYM)
        pts = np.concatenate([pts, ray(im, [0.2, 0.8], [0.2, 0.3], [5.0, 1.0])])
        lands[(0, 5)] = (0, 0)
        refused.append((0, 6))
    return _vertex("exact arguments %dx%d" % (H, W), H, W, SYM, [dict(points=pts)], lands, refused, wins, exact,
                   faults=("half_up",) + (() if (H, W) == (1, 1) else ("seam_wrap",)))


MARGINS = (0.1, 0.3)


def rows_and_seam(d):
    """fp64 rows -d, -1 + d, H - 1 + d, H - d and columns W - 1 + d, W - d: the first of each pair lands, the second is refused."""
    H, W = 5, 10
    im = image(H, W, LIDAR)
    pts = ray(im, [-d, -1 + d, H - 1 + d, H - d, 1.0, 2.0, 3.0], [1.0, 2.0, 3.0, 4.0, W - 1 + d, W - d, 0.0])
    lands = {(0, 0): (0, 1), (0, 2): (H - 1, 3), (0, 4): (1, W - 1), (0, 6): (3, 0)}
    wins = {(0,) + p: i for (_, i), p in lands.items()}
    wins[(0, 2, 0)] = -1                                                # the seam does not wrap
    return _vertex("rows and seam, d=%g" % d, H, W, LIDAR, [dict(points=pts)], lands, [(0, 1), (0, 3), (0, 5)], wins,
                   faults=("seam_wrap",))


def no_range(C):
    """Points without a range, each between two valid rows: r = 0, r^2 underflows, r overflows, NaN, +-inf."""
    H, W = 5, 10
    im = image(H, W, LIDAR)
    base = ray(im, 2.0, 4.0)
    bad = [[0.0, 0.0, 0.0], [1e-23, 0.0, 0.0], [1e-45, 0.0, 0.0], [3e38, 3e38, 0.0]]
    for v in (np.nan, np.inf, -np.inf):
        for a in range(3):
            p = base.astype(np.float64)
            p[a] = v
            bad.append(list(p))
    bad = np.array(bad, dtype=F)
    good = centres(im)[np.arange(len(bad) + 1) * 3]
    pts = np.zeros((2 * len(bad) + 1, C), dtype=F)
    pts[0::2, :3], pts[1::2, :3] = good, bad
    if C == 4:
        pts[:, 3] = np.nan                                              # the fourth column is never read
    lands = {(0, 2 * k): ((3 * k) // W, (3 * k) % W) for k in range(len(good))}
    return _vertex("no range, C=%d" % C, H, W, LIDAR, [dict(points=pts)], lands, [(0, 2 * k + 1) for k in range(len(bad))],
                   {(0,) + p: i for (_, i), p in lands.items()})


def one_ulp_farther(u):
    """u with one coordinate nudged so that the fp32 range grows by exactly one ulp."""
    want = bits32(range32(u)) + 1
    for axis in np.argsort(-np.abs(u)):
        v = u.copy()
        for _ in range(64):
            v[axis] = np.nextafter(v[axis], F(np.inf) * np.sign(v[axis]))
            if bits32(range32(v)) == want:
                return v
    raise AssertionError("no one-ulp neighbour of %r" % (u,))


def zbuffer_ties(boundary):
    """Five groups of two rows on one ray each.  ``boundary``: the two rows lie on either side of row 256, the end of the
    first workgroup of proj_vertex_key_kernel."""
    H, W = 5, 10
    im = image(H, W, LIDAR)
    pairs = [(255 - g, 256 + g) for g in range(5)] if boundary else [(2 * g, 2 * g + 1) for g in range(5)]
    R = 262 if boundary else 12
    u = [ray(im, 1.0 + (g % 3), 1.0 + 2 * g) for g in range(5)]
    pts = np.zeros((R, 3), dtype=F)
    (a, b) = pairs[0]; pts[a], pts[b] = u[0], u[0]                      # identical bits: the lower row
    (a, b) = pairs[1]; pts[a], pts[b] = u[1], F(0.5) * u[1]             # the nearer point at the higher row
    (a, b) = pairs[2]; pts[a], pts[b] = F(2.0) * u[2], u[2]             # the farther point at the lower row
    (a, b) = pairs[3]; pts[a], pts[b] = one_ulp_farther(u[3]), u[3]     # one ulp farther at the lower row
    (a, b) = pairs[4]; pts[a], pts[b] = u[4], one_ulp_farther(u[4])     # one ulp farther at the higher row
    win = [pairs[0][0], pairs[1][1], pairs[2][1], pairs[3][1], pairs[4][0]]
    wins = {(0, 1 + (g % 3), 1 + 2 * g): win[g] for g in range(5)}
    c = _vertex("z-buffer ties%s" % (" across the workgroup boundary" if boundary else ""), H, W, LIDAR, [dict(points=pts)],
                wins=wins, faults=("tie_highest", "ignore_range"))
    c["pairs"] = pairs
    return c


def lengths_case(which):
    """lengths -3, 0, 1 (which = 0) and R, R + 5, 2 (which = 1) on the same six points: the clamp to [0, R]."""
    H, W, R = 5, 10, 6
    im = image(H, W, LIDAR)
    pts = centres(im)[[7, 12, 23, 31, 38, 44]]
    lens = ((-3, 0, 1), (R, R + 5, 2))[which]
    wins = {}
    for s, n in enumerate(lens):
        for i, pix in enumerate([7, 12, 23, 31, 38, 44]):
            wins[(s, pix // W, pix % W)] = i if i < min(max(n, 0), R) else -1
    return _vertex("lengths %s" % (lens,), H, W, LIDAR, [dict(points=pts, length=n) for n in lens], wins=wins)


def keep_case():
    """keep removes exactly the winner (the runner-up wins), and keep all zero (an empty image)."""
    H, W = 5, 10
    im = image(H, W, LIDAR)
    u = ray(im, 2.0, 6.0, 2.0)
    pts = np.stack([u, F(2.0) * u, F(4.0) * u, ray(im, 3.0, 1.0)])
    streams = [dict(points=pts, keep=[1, 1, 1, 1]), dict(points=pts, keep=[0, 1, 1, 1]), dict(points=pts, keep=[0, 0, 0, 0])]
    return _vertex("keep", H, W, LIDAR, streams, wins={(0, 2, 6): 0, (1, 2, 6): 1, (2, 2, 6): -1, (0, 3, 1): 3, (2, 3, 1): -1})


def row_counts(R):
    """R = 1 (far below one workgroup) and R = 257 (one row in a second workgroup, which is the winner)."""
    H, W = 5, 10
    im = image(H, W, LIDAR)
    if R == 1:
        streams = [dict(points=ray(im, 2.0, 3.0)[None], length=1), dict(points=np.zeros((1, 3), dtype=F), length=1)]
        return _vertex("R=1", H, W, LIDAR, streams, wins={(0, 2, 3): 0, (1, 2, 3): -1})
    r = np.random.default_rng(R)
    pts = ray(im, r.integers(0, H, R) + r.uniform(-0.3, 0.3, R), r.integers(0, W, R) + r.uniform(-0.3, 0.3, R),
              r.uniform(3.0, 6.0, R))
    pts[0], pts[R - 1] = F(2.0) * ray(im, 2.0, 3.0, 1.0), ray(im, 2.0, 3.0, 1.0)
    return _vertex("R=%d" % R, H, W, LIDAR, [dict(points=pts)], wins={(0, 2, 3): R - 1})


def vertex_cases():
    return ([exact_arguments(H, W) for H, W in EXACT_SHAPES] + [rows_and_seam(d) for d in MARGINS] + [no_range(3), no_range(4)] +
            [zbuffer_ties(False), zbuffer_ties(True), lengths_case(0), lengths_case(1), keep_case(), row_counts(1),
             row_counts(257)])


# ---- normal map ----------------------------------------------------------------------------------------------------------------

NORMAL_SHAPES = ((1, 1), (1, 40), (9, 1), (2, 33), (9, 33), (8, 32), (17, 65))
SEAMS_X, SEAMS_Y = (31, 32, 63, 64), (7, 8, 15, 16)


def adjugate_normal(m, C):
    """proj_normal (csrc/projective.hpp) restated in fp64 NumPy on moments m (..., 3), C (..., 3, 3) -> (n, det): the adjugate
    over the determinant in the kernel's order of operations, normalised; without the cuts."""
    xx, xy, xz, yy, yz, zz = C[..., 0, 0], C[..., 0, 1], C[..., 0, 2], C[..., 1, 1], C[..., 1, 2], C[..., 2, 2]
    a00, a01, a02 = yy * zz - yz * yz, xz * yz - xy * zz, xy * yz - xz * yy
    a11, a12, a22 = xx * zz - xz * xz, xy * xz - xx * yz, xx * yy - xy * xy
    det = (xx * a00 + xy * a01) + xz * a02
    with np.errstate(all="ignore"):
        n = np.stack([((a00 * m[..., 0] + a01 * m[..., 1]) + a02 * m[..., 2]) / det,
                      ((a01 * m[..., 0] + a11 * m[..., 1]) + a12 * m[..., 2]) / det,
                      ((a02 * m[..., 0] + a12 * m[..., 1]) + a22 * m[..., 2]) / det], axis=-1)
        n = n / np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])[..., None]
    return n, det


def solve_disagreement(vmap, k):
    """The fp64 uncertainty of a normal: the largest component difference between the model's LU solve and the adjugate
    formula on the same moments, over the pixels where the model gives a normal."""
    n, _ = model.normal_map(vmap, k)
    nz = (n != 0).any(axis=-1)
    if not nz.any():
        return 0.0
    m, C = model.moments(np.asarray(vmap, dtype=F), k)
    return float(np.abs(adjugate_normal(m, C)[0][nz] - n[nz]).max())


@functools.lru_cache(maxsize=None)
def occupancy(H, W):
    """A rough surface (ranges 1.5 .. 2.5 m) seen through about 70 % of the pixels; the four corners and the pixels on both
    sides of every tile seam are always filled.  The field of view is steep (30 degrees up), so that the single row of a
    1 x W image lies on a cone far from a plane through the sensor."""
    im = image(H, W, dict(up_fov=30.0, down_fov=-10.0))
    r = np.random.default_rng([H, W])
    v = centres(im, r.uniform(1.5, 2.5, H * W)).reshape(H, W, 3)
    filled = r.uniform(size=(H, W)) < 0.7
    filled[[0, 0, -1, -1], [0, -1, 0, -1]] = True
    filled[:, [x + d for x in SEAMS_X for d in (-1, 0, 1) if x + d < W]] = True       # what a 5 x 5 window reads across a seam
    filled[[y + d for y in SEAMS_Y for d in (-1, 0, 1) if y + d < H], :] = True
    v[~filled] = 0.0
    return dict(edge="occupancy %dx%d" % (H, W), H=H, W=W, vmap=v)


def normal_faults(H, W, k):
    """The planted faults that an H x W image can show to a k x k window: a second tile for the low border; a second tile that
    the window of the last pixel before the seam still reaches for the high border; a next row for the bounds check.  W = 1
    shows none: its points lie in one plane with the sensor, so it has no normals at all."""
    h = k // 2
    if W == 1:
        return ()
    return ((("halo_low",) if W > model.TILE_W or H > model.TILE_H else ()) +
            (("halo_high",) if W > model.TILE_W - 1 + h or H > model.TILE_H - 1 + h else ()) + (("edge_next_row",) if H > 1 else ()))


PLANE_N = np.array([1.0, 0.2, 0.1]) / np.linalg.norm([1.0, 0.2, 0.1])
PLANE_D = dict(far=5.0, near=0.5, cut=0.02)      # det ~ d^6: the first two far above 1e-6, the last far below


@functools.lru_cache(maxsize=None)
def plane(which):
    """The beams of an 8 x 33 image that meet the plane n . p = d at less than 60 degrees from n; the fp64 normal is n."""
    H, W, d = 8, 33, PLANE_D[which]
    im = image(H, W, LIDAR)
    b = model.beams(im)
    c = b @ PLANE_N
    hit = c > 0.5
    v = np.where(hit[:, None], b * (d / np.where(hit, c, 1.0))[:, None], 0.0).astype(F).reshape(H, W, 3)
    return dict(edge="plane d=%g" % d, H=H, W=W, vmap=v, hit=hit.reshape(H, W), n=PLANE_N, d=d)


def lonely():
    """9 x 33: a full 5 x 5 block around an empty centre (zero); a pixel alone and a pixel with one neighbour (one and two
    points: singular moments, zero); a pixel with a neighbour above and one below (three points of one column lie in a plane
    with the sensor: singular, zero); a pixel with two neighbours off that plane (three points span a plane of their own: a
    normal, as the model's)."""
    H, W = 9, 33
    im = image(H, W, LIDAR)
    r = np.random.default_rng(9)
    full = centres(im, r.uniform(1.5, 2.5, H * W)).reshape(H, W, 3)
    v = np.zeros_like(full)
    v[2:7, 2:7] = full[2:7, 2:7]
    v[4, 4] = 0.0                                                       # the empty centre
    for y, x in [(1, 14), (4, 20), (4, 21), (3, 24), (4, 24), (5, 24), (7, 28), (7, 29), (6, 28)]:
        v[y, x] = full[y, x]
    return dict(edge="lonely pixels", H=H, W=W, vmap=v, empty=(4, 4), alone=(1, 14), pair=((4, 20), (4, 21)),
                column=((3, 24), (4, 24), (5, 24)), triple=((7, 28), (7, 29), (6, 28)))


def nan_vertex():
    """A full 9 x 33 image with a NaN in one vertex, and the same image with that vertex emptied."""
    H, W, at = 9, 33, (4, 16)
    im = image(H, W, LIDAR)
    r = np.random.default_rng(11)
    v = centres(im, r.uniform(1.5, 2.5, H * W)).reshape(H, W, 3)
    bad, emptied = v.copy(), v.copy()
    bad[at][1] = np.nan
    emptied[at] = 0.0
    return dict(edge="NaN vertex", H=H, W=W, vmap=bad, emptied=emptied, at=at)


# ---- model build ---------------------------------------------------------------------------------------------------------------

UNITS = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1], [0.6, 0.8, 0], [0, 0.6, -0.8]], dtype=F)
QUARTER = icp.pose(np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), np.array([0.5, -0.25, 0.125]))


def _moved(p, A):
    inv = model.inverse(A)
    return (np.asarray(p, dtype=np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(F)


def _empty_in_band(map_v, A, im, keep=()):
    """Empty every source pixel whose moved point lies within BAND of a boundary (never one of ``keep``: asserted)."""
    p = map_v.reshape(-1, 3)
    near = model.pixels(_moved(p, A), im)[4] < BAND
    assert not near[list(keep)].any()
    p[near] = 0.0


def _build(edge, H, W, fov, map_v, map_n, A, live, **more):
    return dict(edge=edge, H=H, W=W, fov=fov, im=image(H, W, fov), map_v=map_v, map_n=map_n, A=A, live=live, **more)


@functools.lru_cache(maxsize=None)
def collisions(H, W, turned):
    """S = 2, M = 2, every slot live under the same A (I, or a quarter turn about z plus (0.5, -0.25, 0.125)).  In slots
    (0, 0) and (1, 1): the same point at source pixels i < j (src = i); the same point at i < j and a point at half its range
    on the same ray at k > j (src = k); a point at twice the range at l < i (src = i)."""
    im = image(H, W, LIDAR)
    A1 = QUARTER if turned else np.eye(4)
    r = np.random.default_rng([H, W, int(turned)])
    HW = H * W
    map_v = np.stack([centres(im, r.uniform(3.0, 6.0, HW)) for _ in range(4)]).reshape(2, 2, HW, 3)
    plants = {}
    for (s, m) in ((0, 0), (1, 1)):
        p = map_v[s, m]
        moved = _moved(p, A1)
        row, col, _, valid, margin = model.pixels(moved, im)
        alone = np.bincount((row * W + col)[valid], minlength=HW)[row * W + col] == 1
        good = np.flatnonzero(valid & (margin > 0.05) & alone)          # sources that land alone, well inside a pixel
        good = good[(good >= 2) & (good < HW - 4)]
        i1 = good[0]
        i2 = good[good > i1 + 2][0]
        i3 = good[good > i2 + 3][-1]
        j1, j2, k2, l3 = i1 + 1, i2 + 1, i2 + 3, i1 - 1
        assert len({i1, j1, i2, j2, k2, i3, l3}) == 7 and k2 < i3
        p[j1], p[j2] = p[i1], p[i2]
        p[k2] = (np.append(F(0.5) * moved[i2], 1.0).astype(np.float64) @ A1.T)[:3].astype(F)
        p[l3] = (np.append(F(2.0) * moved[i3], 1.0).astype(np.float64) @ A1.T)[:3].astype(F)
        at = lambda i: int((row * W + col)[i])
        plants[(s, m)] = dict(tie=(at(i1), i1, j1), nearer=(at(i2), i2, j2, k2), farther=(at(i3), l3, i3))
    A = np.stack([A1] * 4).reshape(2, 2, 4, 4)
    for s in range(2):
        for m in range(2):
            keep = [i for t in plants.get((s, m), {}).values() for i in t[1:]]
            _empty_in_band(map_v[s, m], A1, im, keep)
    map_n = UNITS[np.arange(2 * 2 * HW) % 5].reshape(2, 2, HW, 3) * (map_v != 0).any(axis=-1, keepdims=True)
    shape = (2, 2, H, W, 3)
    return _build("collisions %dx%d %s" % (H, W, "turned" if turned else "A = I"), H, W, LIDAR, map_v.reshape(shape),
                  map_n.astype(F).reshape(shape), A, np.ones((2, 2), dtype=np.int32), plants=plants, identity=not turned,
                  faults=("tie_highest", "ignore_range"))


SLOT_CASES = {"M=1": (1, (0,)), "M=64": (64, (0, 31, 63)), "all dead": (3, ())}


@functools.lru_cache(maxsize=None)
def slots(which):
    """M = 1; M = 64 (PROJ_MAX_SLOTS) with slots 0, 31 and 63 live; every slot dead.  S = 2, 5 x 10.  A dead slot holds valid
    images and a pose of NaNs, which must not matter."""
    M, alive = SLOT_CASES[which]
    H, W, S = 5, 10, 2
    im = image(H, W, LIDAR)
    r = np.random.default_rng(M)
    map_v = np.stack([centres(im, r.uniform(3.0, 6.0, H * W)) for _ in range(S * M)]).reshape(S, M, H * W, 3)
    live = np.zeros((S, M), dtype=np.int32)
    live[:, list(alive)] = 1
    A = np.full((S, M, 4, 4), np.nan)
    for s in range(S):
        for m in alive:
            A[s, m] = icp.pose(icp.rot(r.normal(size=3), 0.03), r.normal(size=3) * 0.15)
            _empty_in_band(map_v[s, m], A[s, m], im)
    map_n = UNITS[np.arange(S * M * H * W) % 5].reshape(S, M, H * W, 3) * (map_v != 0).any(axis=-1, keepdims=True)
    shape = (S, M, H, W, 3)
    return _build("slots " + which, H, W, LIDAR, map_v.reshape(shape), map_n.astype(F).reshape(shape), A, live, identity=False)


def no_trace():
    """A = I, one slot: a source vertex above the field of view and one that rounds to column W leave no trace; (2, 0), where
    a wrapped seam would put the second, is empty."""
    H, W = 5, 10
    im = image(H, W, LIDAR)
    v = centres(im).reshape(H * W, 3)
    v[2 * W] = 0.0
    v[13], v[27] = ray(im, -2.0, 3.0, 1.0), ray(im, 2.0, W - 0.3, 1.0)  # nearer than whatever else is there
    n = UNITS[np.arange(H * W) % 5] * (v != 0).any(axis=-1, keepdims=True)
    shape = (1, 1, H, W, 3)
    return _build("no trace", H, W, LIDAR, v.reshape(shape), n.astype(F).reshape(shape), np.eye(4).reshape(1, 1, 4, 4),
                  np.ones((1, 1), dtype=np.int32), identity=True, gone=(13, 27), faults=("seam_wrap",))


def build_cases():
    return ([collisions(H, W, t) for (H, W) in ((5, 10), (9, 33)) for t in (False, True)] + [slots(w) for w in SLOT_CASES] +
            [no_trace()])


# ---- accumulate ----------------------------------------------------------------------------------------------------------------

def _acc(edge, H, W, vmap, model_v, model_n, T=None, sigma=0.1, max_dist=1.0, slot=None, pixel=None, faults=(), **more):
    S = vmap.shape[0]
    M = model_v.shape[1]
    T = np.stack([np.eye(4)] * S) if T is None else T
    return dict(edge=edge, H=H, W=W, fov=LIDAR, im=image(H, W, LIDAR), vmap=vmap.reshape(S, H, W, 3),
                model_v=model_v.reshape(S, M, H, W, 3), model_n=model_n.reshape(S, M, H, W, 3), T=T, sigma=sigma,
                max_dist=float(max_dist), slot=slot or {}, pixel=pixel or {}, faults=tuple(faults), **more)


def _blank(S, M, HW):
    return np.zeros((S, HW, 3), dtype=F), np.zeros((S, M, HW, 3), dtype=F), np.zeros((S, M, HW, 3), dtype=F)


def _dx(d):
    return np.array([d, 0.0, 0.0], dtype=F)


def slot_ties():
    """Candidates at q +- (0.25, 0, 0) in slots 0 and 2 (both ways round): slot 0.  A nearer candidate in slot 2: slot 2."""
    H, W = 5, 10
    q = short(centres(image(H, W, LIDAR)))
    v, mv, mn = _blank(1, 3, H * W)
    for i in (3, 7, 12, 20):
        v[0, i] = q[i]
    mv[0, 0, 3], mv[0, 2, 3] = q[3] + _dx(0.25), q[3] - _dx(0.25)
    mv[0, 0, 7], mv[0, 2, 7] = q[7] - _dx(0.25), q[7] + _dx(0.25)
    mv[0, 0, 12], mv[0, 2, 12] = q[12] + _dx(0.25), q[12] + _dx(0.125)
    mv[0, 1, 20] = q[20] + np.array([0.0, 0.25, 0.0], dtype=F)
    mn[(mv != 0).any(axis=-1)] = UNITS[3]
    return _acc("slot ties", H, W, v, mv, mn, slot={(0, 3): 0, (0, 7): 0, (0, 12): 2, (0, 20): 1}, faults=("slot_tie_le",))


MAX_DISTS = {"equal": 0.5, "below": float(np.nextafter(F(0.5), F(0.0))), "zero": 0.0}


def max_dist_edge(which):
    """Candidates at distance 0.5, 0 and 0.25 exactly, against max_dist = 0.5, the fp32 number below 0.5, and 0."""
    H, W = 5, 10
    q = short(centres(image(H, W, LIDAR)))
    v, mv, mn = _blank(1, 1, H * W)
    for i, d in ((3, 0.5), (7, 0.0), (12, 0.25)):
        v[0, i], mv[0, 0, i], mn[0, 0, i] = q[i], q[i] + _dx(d), UNITS[3]
    want = {"equal": (0, 0, 0), "below": (-1, 0, 0), "zero": (-1, 0, -1)}[which]
    return _acc("max_dist " + which, H, W, v, mv, mn, max_dist=MAX_DISTS[which], slot=dict(zip(((0, 3), (0, 7), (0, 12)), want)),
                faults=() if which == "below" else ("max_dist_lt",))


def refusals():
    """The nearest slot without a normal; a NaN model vertex in the lower slot; a NaN source vertex; a source vertex above
    the field of view, on the refused seam column (a candidate waits where a wrapped seam would look), an empty source
    pixel; and one ordinary pair."""
    H, W = 5, 10
    im = image(H, W, LIDAR)
    q = short(centres(im))
    v, mv, mn = _blank(1, 2, H * W)
    for i in (3, 7, 12, 40):
        v[0, i] = q[i]
    mv[0, 0, 3], mv[0, 1, 3], mn[0, 1, 3] = q[3] + _dx(0.125), q[3] + _dx(0.25), UNITS[0]
    mv[0, 0, 7], mn[0, 0, 7], mv[0, 1, 7], mn[0, 1, 7] = q[7], UNITS[0], q[7] + _dx(0.125), UNITS[0]
    mv[0, 0, 7, 1] = np.nan
    v[0, 12, 2] = np.nan
    mv[0, 0, 12], mn[0, 0, 12] = q[12], UNITS[0]
    v[0, 31], v[0, 25] = ray(im, -2.0, 3.0), ray(im, 2.0, W - 0.3)
    mv[0, 0, 20], mn[0, 0, 20] = v[0, 25] + _dx(0.125), UNITS[0]        # (2, 0): where a wrapped seam would look
    mv[0, 0, 40], mn[0, 0, 40] = q[40] + _dx(0.125), UNITS[3]
    return _acc("refusals", H, W, v, mv, mn, slot={(0, 3): -1, (0, 7): -1, (0, 12): -1, (0, 31): -1, (0, 25): -1, (0, 20): -1,
                                                    (0, 40): 0},
                pixel={(0, 3): 3, (0, 7): 7, (0, 12): -1, (0, 31): -1, (0, 25): -1, (0, 20): -1, (0, 40): 40},
                faults=("zero_normal_skip", "seam_wrap"))


def translated():
    """T = a translation by (0.5, 0, 0), exact on short mantissas: every source looks at the pixel of its moved point, where
    a candidate at q + (0, 0.125, 0) waits; sources whose moved point lies in the band are emptied."""
    H, W = 5, 10
    im = image(H, W, LIDAR)
    p = short(centres(im, 2.0))
    T = icp.pose(np.eye(3), np.array([0.5, 0.0, 0.0]))[None]
    q = p + _dx(0.5)
    row, col, _, valid, margin = model.pixels(q, im)
    p[margin < BAND] = 0.0
    v, mv, mn = _blank(1, 1, H * W)
    v[0] = p
    for i in np.flatnonzero(valid & (margin >= BAND)):
        at = row[i] * W + col[i]
        mv[0, 0, at], mn[0, 0, at] = q[i] + np.array([0.0, 0.125, 0.0], dtype=F), UNITS[i % 5]
    return _acc("translated", H, W, v, mv, mn, T=T, moved_off=int((np.flatnonzero(valid) != (row * W + col)[valid]).sum()),
                left=int((~valid).sum()))


REDUCTION_SHAPES = ((1, 1), (5, 51), (8, 32), (1, 257))             # HW = 1, 255, 256, 257 around ICP_ACC_THREADS = 256


def reductions(H, W):
    """Stream 0: pairs in the first and the last pixel only; stream 1: in every pixel; stream 2: none."""
    HW = H * W
    q = short(centres(image(H, W, LIDAR)))
    v, mv, mn = _blank(3, 1, HW)
    v[:] = q
    v[0, 1:HW - 1] = 0.0
    mv[:2, 0] = q + _dx(0.125)
    mn[:2, 0] = UNITS[np.arange(HW) % 5]
    mv[0, 0, 1:HW - 1] = 0.0
    slot = {(0, 0): 0, (0, HW - 1): 0, (1, 0): 0, (1, HW - 1): 0, (1, HW // 2): 0, (2, 0): -1, (2, HW - 1): -1}
    return _acc("reductions HW=%d" % HW, H, W, v, mv, mn, slot=slot, pairs=(min(2, HW), HW, 0))


def accumulate_cases():
    return ([slot_ties()] + [max_dist_edge(w) for w in MAX_DISTS] + [refusals(), translated()] +
            [reductions(H, W) for H, W in REDUCTION_SHAPES])


# ---- map push ------------------------------------------------------------------------------------------------------------------

PUSH_M = (1, 2, 64)


def push(M, which):
    """S = 3, 2 x 3 images; cursors -5, 0, M - 1 (which = 0) and M, 99, 0 (which = 1): the clamp, then the wrap after M - 1.
    Every slot holds its own random images and pose; about half are dead."""
    S, H, W = 3, 2, 3
    r = np.random.default_rng([M, which])
    f = lambda *s: r.normal(size=s).astype(F)
    rigid = lambda: icp.pose(icp.rot(r.normal(size=3), r.uniform(0.1, 1.0)), r.normal(size=3))
    live = (r.uniform(size=(S, M)) < 0.5).astype(np.int32)
    live[:, -1], live[0, 0] = 1, 0
    return dict(edge="push M=%d cursors %d" % (M, which), M=M, T=np.stack([rigid() for _ in range(S)]), vmap=f(S, H, W, 3),
                nmap=f(S, H, W, 3), map_v=f(S, M, H, W, 3), map_n=f(S, M, H, W, 3),
                A=np.stack([rigid() for _ in range(S * M)]).reshape(S, M, 4, 4), live=live,
                cursor=np.array(((-5, 0, M - 1), (M, 99, 0))[which], dtype=np.int32),
                target=((0, 0, M - 1), (M - 1, M - 1, 0))[which], faults=("no_cursor_clamp",))


def push_cases():
    return [push(M, w) for M in PUSH_M for w in (0, 1)]
