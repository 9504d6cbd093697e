"""Planted cases of the map localiser, in NumPy alone.  A case is a dict: the map as keyframe clouds
(K, n, 3) at poses (K, 4, 4) with its voxel size, the radius, world queries ``q``, the pairing settings, the planted fault
of tests/map_localize_model.py under which the case's answer changes, and ``edge``: what the case must reach.
tests/test_map_localize_cpu.py proves both on the model; tests/test_gpu_map_localize.py runs the cases through the
kernels.  Coordinates are small integers and v = 1 wherever a distance has to be exact."""
import functools

import numpy as np

import icp_model as icp
import map_localize_model as M

F = np.float32
ROWS = 64                                        # rows per keyframe of the planted maps (the smallest the tests build)
MARKER = (1355969, -5175622, 0)                  # the voxel whose hash is the table's empty marker
EDGE_V = 2.0 ** 30 / (2.0 ** 31 - 1.0)           # float32 2^30 divided by it lies in voxel 2^31 - 1


def _cloud(points, n=ROWS):
    """One keyframe of n rows that holds ``points`` first; the padding repeats the first point (its voxel is taken)."""
    pts = np.asarray(points, dtype=F).reshape(-1, 3)
    assert 1 <= len(pts) <= n
    return np.concatenate([pts, np.repeat(pts[:1], n - len(pts), axis=0)])[None]


def _case(name, points, q, v=1.0, R=1, fault=None, edge=None, min_neighbours=5, max_dist=None, n=ROWS):
    return dict(name=name, clouds=_cloud(points, n), poses=np.eye(4)[None], v=v, R=R, q=np.asarray(q, dtype=F).reshape(-1, 3),
                fault=fault, edge=edge, min_neighbours=min_neighbours,
                max_dist=M.largest_max_dist(R, v) if max_dist is None else max_dist)


def patch(k):
    """k <= 9 points of the plane z = 0, one per voxel around the origin, never collinear from the third on."""
    cells = [(0, 0), (1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1)]
    return [(x, y, 0.0) for x, y in cells[:k]]


@functools.lru_cache(maxsize=None)
def table():
    one = F(1.0)
    out = [
        # two candidates at the same fp32 distance: the first in dz, dy, dx order wins
        _case("tie-x", [(-1, 0, 0), (1, 0, 0)], [(0, 0, 0)], fault="tie_le", edge="tie"),
        _case("tie-order", [(1, 0, -1), (-1, 0, 1)], [(0, 0, 0)], fault="order_swapped", edge="tie"),
        # d on both fp32 neighbours of max_dist = 1: the nine points of a plane one voxel below the query
        _case("max-dist", patch(9), [(0, 0, np.nextafter(one, F(0))), (0, 0, one), (0, 0, np.nextafter(one, F(2)))],
              fault="max_dist_strict", edge="max_dist"),
        # min_neighbours and one fewer
        _case("count-5", patch(5), [(0, 0, 0.25)], fault="count_off_by_one", edge="count_eq"),
        _case("count-4", patch(4), [(0, 0, 0.25)], edge="count_below"),
        # five collinear points (radius 2 reaches them all): enough neighbours, no plane
        _case("collinear", [(i, 0, 0) for i in range(-2, 3)], [(0, 0, 0.25)], R=2, edge="collinear"),
        # one point is a neighbourhood of duplicates of itself
        _case("single", [(0, 0, 0)], [(0, 0, 0.25)], min_neighbours=1, edge="single"),
        # queries that are no queries, and one far from everything
        _case("unusable", patch(9), [(np.nan, 0, 0), (0, np.inf, 0), (3e38, 0, 0), (0, 0, -3e38), (500, 500, 500)],
              edge="unusable"),
        # the voxel next to +2^31 and to -2^31: the neighbours past the limit are skipped
        _case("range-edge", [(2.0 ** 30, 0, 0), (-2.0 ** 30, 0, 0)], [(2.0 ** 30, 0, 0), (-2.0 ** 30, 0, 0)], v=EDGE_V,
              fault="no_range_skip", edge="range"),
        # the voxel whose key is the empty marker: it lives in slot T
        _case("marker", [MARKER, (MARKER[0] + 1, MARKER[1], 0)], [MARKER, (MARKER[0] + 1, MARKER[1], 0)], edge="marker"),
    ]
    return out


def stale():
    """A map, and the same bank at shifted poses: what an index of the first finds in the second."""
    r = np.random.default_rng(31)
    clouds = r.uniform(-3.0, 3.0, (3, 96, 3)).astype(F)
    clouds[:, :, 2] *= 0.1
    before = np.stack([icp.pose(np.eye(3), [0.1 * k, 0.0, 0.0]) for k in range(3)])
    after = np.stack([icp.pose(icp.rot([0, 0, 1], 0.02 * (k + 1)), [0.1 * k + 0.37, -0.21, 0.05]) for k in range(3)])
    after[0] = before[0]                         # the first keyframe stays: its points keep voxel and rank, and stay findable
    q = (clouds.reshape(-1, 3)[::3] + r.normal(0.0, 0.1, (96, 3))).astype(F)
    return dict(clouds=clouds, before=before, after=after, v=0.3, q=q)


def scene(frames=6, n=1024, seed=3):
    """The box room of icp_cases: ``frames - 1`` keyframes at their true world poses and the last frame as the query, with
    guesses off by 2 degrees and 0.3 m -> dict(clouds, poses, cloud, truth, guesses)."""
    clouds, rel = icp.room(seed, frames, n)
    world = [np.eye(4)]
    for k in range(1, frames):
        world.append(world[-1] @ rel[k])
    world = np.stack(world)
    truth = world[-1]
    guesses = [icp.perturbed(truth, 2.0, 0.3), icp.perturbed(truth, -2.0, -0.3)]
    return dict(clouds=clouds[:-1], poses=world[:-1], cloud=clouds[-1], truth=truth, guesses=guesses, v=0.3)


SCENE_RADIUS = 2                                 # the radius at which the fp64 model meets the scene's condition (see the CPU test)


def random_map(K, n, v, seed=7):
    """K keyframes of n rows on two noisy planes around the origin, at small poses: a map dense enough for planes."""
    r = np.random.default_rng([seed, K, n])
    clouds = r.uniform(-2.0, 2.0, (K, n, 3)) * (4.0 * v)
    clouds[:, : n // 2, 2] = 0.2 * clouds[:, : n // 2, 0] + r.normal(0.0, 0.02 * v, (K, n // 2))
    clouds[:, n // 2:, 0] = -0.3 * clouds[:, n // 2:, 1] + r.normal(0.0, 0.02 * v, (K, n - n // 2))
    poses = np.stack([icp.pose(icp.rot(r.normal(size=3), 0.05), r.normal(size=3) * v) for _ in range(K)])
    return clouds.astype(F), poses


def queries(points, n, v, R, seed=5):
    """n world queries for a map: near its points, on the faces of their voxel blocks, far away, and the unusable ones at
    the workgroup edges (rows 0, 255, 256, 511, 512 where n reaches them)."""
    r = np.random.default_rng([seed, n, R])
    pts = np.asarray(points, dtype=F).reshape(-1, 3)
    q = (pts[r.integers(0, len(pts), n)] + r.normal(0.0, 0.4 * v, (n, 3))).astype(F)
    face = np.rint(pts[r.integers(0, len(pts), n)].astype(np.float64) / v)
    on = (face + np.array([R + 0.5, 0.0, -(R + 0.5)])) * v                 # half a voxel past the block on two axes
    q[1::5] = on[1::5].astype(F)
    q[2::7] = r.uniform(-900.0, 900.0, (len(q[2::7]), 3)).astype(F)
    q[3::11] = pts[r.integers(0, len(pts), len(q[3::11]))]                 # a stored point itself: d = 0
    bad = [(np.nan, 0, 0), (0, -np.inf, 0), (3e38, 0, 0)]
    for j, i in enumerate((0, 255, 256, 511, 512)):
        if i < n:
            q[i] = bad[j % 3]
    return q
