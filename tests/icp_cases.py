"""Edge cases of the knn refiner's own ops (csrc/icp.hip on csrc/icp.hpp), built in NumPy alone on
tests/icp_model.py: every case is a dict of planted inputs of one op.  tests/test_icp_cases_cpu.py proves on the model that
each case holds what its name says; tests/test_gpu_icp_edges.py runs the same cases through the kernels, every output a
view into a larger allocation whose borders must stay intact.

What makes an edge decidable to the bit: products of short integers are exact in fp64 (the lattice planes of the normals),
``q`` is an input of the accumulate kernel, so a residual can be planted as a difference of two fp32 numbers against the
normal (0, 0, 1) (|r| == sigma), and a diagonal system with power-of-two pivots solves without a rounding (|delta| ==
threshold).  Out-of-range indices, NaNs and ties are planted in stream 1 of 3 only: a kernel that wrongly used them would
read the neighbouring streams' rows, and fail the comparison, instead of leaving the allocation."""
import functools
import itertools

import numpy as np

import icp_model as model

F = np.float32
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
NAN64 = np.array([0x7FF8DEAD0000BEEF], dtype=np.uint64).view(np.float64)[0]      # the pre-fill of every fp64 output
NAN32 = np.array([0x7FC0BEEF], dtype=np.uint32).view(np.float32)[0]
SENTINEL_I32 = 0x5A5A5A5A                                                        # the pre-fill of every int32 output
GUARD_BYTE, GUARD_BYTES = 0xA5, 256
IDLE = 8


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def poses(r, k, angle=0.3, shift=1.0):
    return np.stack([model.pose(model.rot(r.normal(size=3), r.uniform(0.0, angle)), r.normal(size=3) * shift)
                     for _ in range(k)])


# ---- normals -------------------------------------------------------------------------------------------------------------------

NORMAL_SHAPES = ((64, 63), (65, 10))
PLANE = np.array([1.0, 2.0, 2.0]) / 3.0          # the lattice plane's unit normal; (2, -1, 0) and (2, 0, -1) span the plane


def _lattice(n, origin):
    i = np.arange(n)
    return (np.asarray(origin, dtype=np.float64) + np.outer(i % 8, [2.0, -1.0, 0.0]) + np.outer(i // 8, [2.0, 0.0, -1.0])).astype(F)


def _rank(n, k, ratio):
    """A line along x with spacing 1; y alternates by ``ratio`` times the neighbourhood's first extent, z moves an eighth of
    that about 5: the second extent of every neighbourhood is ``ratio`` of its first."""
    i = np.arange(n)
    amp = ratio * min(k, n - 1)
    return np.stack([i * 1.0, amp * (i % 2), 5.0 + 0.125 * amp * ((i // 2) % 2)], axis=1).astype(F)


@functools.lru_cache(maxsize=None)
def normals_cases():
    out = []
    for n, k in NORMAL_SHAPES:
        tag = "n%d-k%d" % (n, k)
        out.append(dict(name="planar-" + tag, edge="planar", n=n, k=k, xyz=_lattice(n, (3.0, 6.0, 6.0)), plane=PLANE, plane_int=np.array([1.0, 2.0, 2.0])))
        i = np.arange(n)
        flat = np.stack([i % 8 - 4.0, i // 8 - 4.0, np.zeros(n)], axis=1).astype(F)           # z = 0: n . y == 0 exactly
        out.append(dict(name="origin-" + tag, edge="origin", n=n, k=k, xyz=flat, plane=np.array([0.0, 0.0, 1.0]), plane_int=np.array([0.0, 0.0, 1.0])))
        out.append(dict(name="rank-below-" + tag, edge="rank_below", n=n, k=k, xyz=_rank(n, k, 3e-6)))
        out.append(dict(name="rank-above-" + tag, edge="rank_above", n=n, k=k, xyz=_rank(n, k, 3e-5)))
        big = (model.normals_cloud(1, n, seed=BIG_SEEDS[(n, k)])[0].astype(np.float64) + np.array([1.0e4, -1.0e4, 5.0e3])).astype(F)
        out.append(dict(name="big-" + tag, edge="big", n=n, k=k, xyz=big))
        clean = model.normals_cloud(1, n, seed=NAN_SEEDS[(n, k)])[0]
        out.append(dict(name="nan-" + tag, edge="nan", n=n, k=k, xyz=clean, nan_point=n // 3))
    return out


BIG_SEEDS = {(64, 63): 5, (65, 10): 5}           # seeds for which the model leaves out at most GAP_CAP of the cloud
NAN_SEEDS = {(64, 63): 5, (65, 10): 5}


def nan_cloud(c):
    """The case's cloud with its one NaN point, and the rows that must come out zero given the neighbour lists ``idx``
    (n, k + 1) of the CLEAN cloud: the kernel takes the lists as an input, so the lists stay those of the clean cloud and
    no search ever sees a NaN."""
    x = c["xyz"].copy()
    x[c["nan_point"]] = np.nan
    return x


def nan_rows(c, idx):
    hit = (idx[:, 1:] == c["nan_point"]).any(axis=1)
    hit[c["nan_point"]] = True
    return hit


# ---- queries -------------------------------------------------------------------------------------------------------------------

QUERY_SHAPES = [(S, M, n) for n in (1, 255, 256, 257) for S, M in ((2, 1), (1, 64))] + [(3, 64, 257)]      # grid.y = 192


@functools.lru_cache(maxsize=None)
def queries_case(S, M, n):
    r = np.random.default_rng([41, S, M, n])
    return dict(S=S, M=M, n=n, p=r.uniform(-40.0, 40.0, (S, n, 3)).astype(F), A=poses(r, S * M, 3.0, 5.0).reshape(S, M, 4, 4),
                T=poses(r, S, 0.1), active=np.array([(s + 1) % 2 for s in range(S)], dtype=np.int32))


# ---- accumulate ------------------------------------------------------------------------------------------------------------------

ACC_N = (1, 63, 64, 65, 255, 256, 257, 513)
ACC_M = (1, 3, 64)


def accumulate_groups(p, q32, idx, dist, map_xyz, map_normals, live, R, T, sigma, max_dist):
    """icp_model.accumulate restricted to the points [256 g, 256 g + 256) of one stream -> (sum (G, 32), mag (G, 32)): what
    each workgroup of icp_accumulate_kernel stores in its own row."""
    n = p.shape[0]
    rows = [model.accumulate(p, q32, idx, dist, map_xyz, map_normals, live, R, T, sigma, max_dist,
                             points=slice(256 * g, min(n, 256 * g + 256))) for g in range((n + 255) // 256)]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


ACC_KEYS = ("p", "q", "idx", "dist", "map_xyz", "map_normals", "live", "R", "T")


def case_groups(c, s):
    return accumulate_groups(*[c[k][s] for k in ACC_KEYS], c["sigma"], c["max_dist"])


def _acc_inputs(S, M, n, seed, sigma=0.5, max_dist=1.0):
    r = np.random.default_rng([seed, S, M, n])
    p = r.uniform(-5.0, 5.0, (S, n, 3)).astype(F)
    T = poses(r, S, 0.05, 0.1)
    A = poses(r, S * M).reshape(S, M, 4, 4)
    R = np.ascontiguousarray(np.transpose(A[:, :, :3, :3], (0, 1, 3, 2)))
    q = np.stack([model.queries(A[s], p[s], T[s])[1] for s in range(S)])
    idx = r.integers(0, n, (S, M, n)).astype(np.int32)
    dist = r.uniform(0.0, 1.4, (S, M, n)).astype(F)
    nrm = r.normal(size=(S, M, n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(F)
    nrm[:, :, 5::17] = 0.0
    scale = np.where(r.random((S, M, n, 1)) < 0.5, 0.1, 2.0)
    map_xyz = r.uniform(-5.0, 5.0, (S, M, n, 3)).astype(F)
    for s in range(S):
        for m in range(M):
            map_xyz[s, m, idx[s, m]] = q[s, m] + (scale[s, m] * r.normal(size=(n, 3))).astype(F)
    return dict(S=S, M=M, n=n, p=p, q=q, idx=idx, dist=dist, map_xyz=map_xyz, map_normals=nrm,
                live=np.ones((S, M), dtype=np.int32), R=R, T=T, sigma=sigma, max_dist=max_dist, aims={}, all=())


def _shape_case(M, n):
    """The general case of a shape: in stream 1 ties between slots (the lower must win), dist == max_dist exactly and, for
    M >= 3, a dead slot 1 full of NaNs and wild indices."""
    c = _acc_inputs(3, M, n, 61)
    c["name"] = "shape-n%d-M%d" % (n, M)
    c["dist"][1, 0, 1::7] = F(1.0)
    if M >= 3:
        c["live"][1, 1] = 0
        c["dist"][1, 1], c["map_xyz"][1, 1], c["map_normals"][1, 1], c["idx"][1, 1] = np.nan, np.nan, np.nan, 1 << 30
        c["dist"][1, 2, ::3] = c["dist"][1, 0, ::3]
        c["dist"][1, 2, 1::7] = F(1.0)
        c["dist"][1, 3:, ::3] = F(1.3)
        c["aims"] = {"tie": 1, "dist_eq_max": 1} if n >= 8 else {}
    return c


def _quiet(c, s=1):
    """Every point of stream s is rejected by its distance until a case plants a pair."""
    c["dist"][s] = F(2.0)


def _plant(c, i, m=None, r=None, s=1, dist=0.25):
    """Point i of stream s pairs with slot m (the middle slot by default); r: plant the residual exactly, through q, the
    map point (1, 2, 0) and the normal (0, 0, 1)."""
    m = c["M"] // 2 if m is None else m
    c["dist"][s, m, i] = F(dist)
    j = c["idx"][s, m, i]
    if r is not None:
        c["map_xyz"][s, m, j], c["map_normals"][s, m, j] = (1.0, 2.0, 0.0), (0.0, 0.0, 1.0)
        c["q"][s, m, i] = (1.0, 2.0, r)
    elif not c["map_normals"][s, m, j].any():
        c["map_normals"][s, m, j] = (0.0, 0.6, 0.8)


def _edge(name, M, n, aims, all_=(), **kw):
    c = _acc_inputs(3, M, n, 67, **kw)
    c.update(name=name, aims=aims, all=all_)
    return c


def _residuals(name, sigma, rs, aim):
    """One pair per residual in stream 1, each with its own map point (the indices are made distinct first)."""
    c = _edge(name, 3, 257, {aim: 1}, sigma=sigma)
    _quiet(c)
    at = [3, 70, 140, 200, 255, 256, 9, 77][:len(rs)]
    c["idx"][1, 1, at] = np.arange(len(rs)) + 11
    for i, r in zip(at, rs):
        _plant(c, i, r=F(r))
    return c


@functools.lru_cache(maxsize=None)
def accumulate_cases():
    out = [_shape_case(M, n) for n in ACC_N for M in ACC_M]
    c = _edge("all-dead", 3, 257, {"dead": 0}, all_=("dead",))
    c["live"][:] = 0
    out.append(c)
    c = _edge("dead-stream", 3, 257, {"dead": 1}, all_=("dead",))
    c["live"][1] = 0
    out.append(c)
    for name, n, i in (("single-first", 257, 0), ("single-last-n257", 257, 256), ("single-last-n513", 513, 512),
                       ("single-last-n255", 255, 254), ("single-only-n1", 1, 0)):
        c = _edge(name, 3, n, {"used": 1}, all_=("used",) if n == 1 else ())
        _quiet(c)
        _plant(c, i)
        c["only"] = i
        out.append(c)
    for w in range(4):                                   # one pair in wave w alone: a butterfly or a wave sum that drops a wave
        c = _edge("wave-%d" % w, 3, 256, {"used": 1})
        _quiet(c)
        _plant(c, 64 * w + 37)
        c["only"] = 64 * w + 37
        out.append(c)
    c = _edge("idx-rejected", 3, 257, {"index": 1})
    _quiet(c)
    for i, j in enumerate((-1, 257, INT_MIN, INT_MAX)):
        for at in (i, 100 + i, 253 + i):                 # 256: the one point of the second workgroup
            _plant(c, at)
            c["idx"][1, 1, at] = j
    for at in (8, 9, 200):
        _plant(c, at)
    out.append(c)
    c = _edge("nan-first-slot", 3, 257, {"nan_first": 1, "nan_later": 1})
    c["dist"][1, 0, :20], c["dist"][1, 1, :20] = np.nan, F(0.1)          # rejected although slot 1 is finite
    c["dist"][1, 0, 20:40], c["dist"][1, 1, 20:40], c["dist"][1, 2, 20:40] = F(0.3), np.nan, F(0.5)    # slot 0 pairs
    c["dist"][1, 0, 256], c["dist"][1, 1, 256] = np.nan, F(0.1)
    out.append(c)
    c = _edge("dist-inf", 3, 257, {"inf_first": 1, "inf_all": 1})
    c["dist"][1, 0, :20], c["dist"][1, 1, :20], c["dist"][1, 2, :20] = np.inf, F(0.2), F(0.4)    # a later finite slot wins
    c["dist"][1, :, 20:40] = np.inf                                                               # rejected
    out.append(c)
    c = _edge("dist-inf-max-dist-inf", 3, 257, {"inf_all": 1}, max_dist=float("inf"))
    c["dist"][1, :, 20:40] = np.inf                                                               # inf <= inf: slot 0 pairs
    out.append(c)
    c = _edge("max-dist-zero", 3, 257, {"dist_eq_max": 1, "dist_above": 1}, max_dist=0.0)
    c["dist"][1, 1, :10] = F(0.0)
    c["dist"][1, 1, 10:20] = np.nextafter(F(0.0), F(1.0))
    c["dist"][1, 1, 256] = F(0.0)
    out.append(c)
    s3 = float(F(0.3))
    out.append(_residuals("r-equals-sigma", s3, (s3, -s3, np.nextafter(F(0.3), F(0)), np.nextafter(F(0.3), F(1))), "sigma_bit"))
    out.append(_residuals("sigma-below-clamp", 5e-5, (6e-5, 1e-4, 2e-4, -6e-5, -1e-4, -2e-4, 4e-5), "clamp"))
    out.append(_residuals("r-zero", 0.5, (0.0, -0.0, 0.25), "r_zero"))
    return out


def branches(c, s):
    """Per point of stream s, which branch of icp_accumulate_kernel it takes (boolean arrays), and its residual."""
    dist, live, idx = c["dist"][s], c["live"][s], c["idx"][s]
    M, n = dist.shape
    slot, ok = model.choose(dist, live, c["max_dist"])
    at = np.arange(n)
    sl = np.maximum(slot, 0)
    bd = dist[sl, at]
    j = idx[sl, at].astype(np.int64)
    inb = (j >= 0) & (j < n)
    jj = np.where(inb, j, 0)
    nn = c["map_normals"][s][sl, jj]
    used = ok & inb & (nn != 0).any(axis=1)
    d = c["q"][s][sl, at].astype(np.float64) - c["map_xyz"][s][sl, jj].astype(np.float64)
    nd = nn.astype(np.float64)
    with np.errstate(invalid="ignore"):
        r = (nd[:, 0] * d[:, 0] + nd[:, 1] * d[:, 1]) + nd[:, 2] * d[:, 2]                # the kernel's order
        alive = np.flatnonzero(live)
        if alive.size == 0:
            alive, slot = np.array([0]), np.full((n,), -1)               # nothing below is true of a point without a slot
        first, later = dist[alive[0]], dist[alive[1:]]
        ar = np.abs(r)
        equal = dist[alive] == bd[None]
        lowest = alive[np.argmax(equal, axis=0)]                         # the lowest live slot that holds the chosen distance
        return dict(
            slot=slot, used=used, r=r, dead=slot < 0, index=ok & ~inb, zero_normal=ok & inb & ~used,
            nan_first=np.isnan(first) & np.isfinite(later).any(axis=0) & (slot >= 0) & ~ok,
            nan_later=used & np.isnan(later).any(axis=0),
            inf_first=used & np.isinf(first) & (slot > alive[0]),
            inf_all=np.isinf(bd) & (slot >= 0), tie=used & (equal.sum(axis=0) > 1) & (slot == lowest),
            dist_eq_max=used & (bd == F(c["max_dist"])),
            dist_above=(slot >= 0) & (bd > F(c["max_dist"])) & (bd <= np.nextafter(F(c["max_dist"]), F(np.inf))),
            sigma_bit=used & (ar == c["sigma"]), clamp=used & (ar >= c["sigma"]) & (ar <= model.HUBER_CLAMP),
            above_clamp=used & (ar >= c["sigma"]) & (ar > model.HUBER_CLAMP), r_zero=used & (r == 0.0))


# ---- solve -------------------------------------------------------------------------------------------------------------------------

SOLVE_S = (1, 31, 32, 33, 65)
SOLVE_G = (1, 2, 64)
JUNK_ROW3 = np.array([1e30, np.nan, -7.0, 0.5])
STEP_345 = np.array([0.0, 0.0, 0.0, 3.0, 4.0, 0.0]) * 2.0 ** -10          # |step| = 5 * 2^-10 without a rounding
NEAR_PI = (np.pi - 5e-7) * PLANE


def _diag_row(step):
    """sw = 1, H = 4 I, g = -4 step: with damping 0 the pivots are 2 and the solve is exact: delta = step."""
    row = np.zeros((model.ROW,))
    for e, (a, b) in enumerate(model.UPPER):
        row[model.H0 + e] = 4.0 if a == b else 0.0
    row[model.G0:model.G0 + 6] = -4.0 * np.asarray(step)
    row[model.SW], row[model.COST], row[model.PAIRS] = 1.0, 0.0625, 400.0
    return row


@functools.lru_cache(maxsize=None)
def _one_pair_row():
    """The row of a single pair whose point sits on the sensor (p = 0, T = I): J = (0, 0, 0, n) with n = (0, 0, 1), so H has
    one non-zero entry.  Damping 0: the first pivot is 0.  Damping 1e-6: a diagonal system, solved to rounding.  (A pair
    with a general J gives a system of condition |J|^2 / damping ~ 1e7, whose solution two Cholesky codes agree on to 1e-9
    at best: ``_general_pair_row`` is that pair, with a bound of its own.)"""
    one = lambda a: np.asarray(a)[None]
    row, _ = model.accumulate(np.zeros((1, 3), dtype=F), one(np.array([[1.0, 2.0, 0.25]], dtype=F)), np.zeros((1, 1), dtype=np.int32),
                              np.zeros((1, 1), dtype=F), one(np.array([[1.0, 2.0, 0.0]], dtype=F)),
                              one(np.array([[0.0, 0.0, 1.0]], dtype=F)), np.ones((1,), dtype=np.int32), one(np.eye(3)), np.eye(4),
                              0.5, 1.0)
    return row


@functools.lru_cache(maxsize=None)
def _general_pair_row():
    """The row of a single pair with a general Jacobian, for damping = 1e-6 only: H / sw = J J^T has rank one, so the damped
    system has condition (|J|^2 + damping) / damping, about 1e7 (``solve_tolerance`` has the bound that follows from it).
    Under damping 0 its second pivot is zero up to rounding, of either sign: no case."""
    one = lambda a: np.asarray(a)[None]
    T = poses(np.random.default_rng(97), 1, 0.3)[0]
    row, _ = model.accumulate(np.array([[1.5, -2.25, 0.75]], dtype=F), one(np.array([[1.25, 1.5, 0.75]], dtype=F)),
                              np.zeros((1, 1), dtype=np.int32), np.zeros((1, 1), dtype=F), one(np.array([[1.0, 2.0, 0.5]], dtype=F)),
                              one(np.array([[0.36, -0.48, 0.8]], dtype=F)), np.ones((1,), dtype=np.int32), one(model.rot([1.0, 2.0, 3.0], 0.2)),
                              T, 0.5, 1.0)
    return row


def solve_tolerance(kind, row, damping):
    """The norm-wise relative bound on delta for a stream of a solve case: the project's 1e-10, except for the general single
    pair.  There the kernel's Cholesky and the model's are both backward stable, so each is off the exact solution by at
    most c n eps64 cond with n = 6 and a small constant c; 64 eps64 cond covers the two together.  cond = (trace(H / sw) +
    damping) / damping: the one non-zero eigenvalue of J J^T is its trace."""
    if kind != "one_pair_general":
        return 1e-10
    trace = sum(row[model.H0 + e] for e, (a, b) in enumerate(model.UPPER) if a == b) / row[model.SW]
    return 64.0 * model.EPS64 * (trace + damping) / damping


@functools.lru_cache(maxsize=None)
def _rows(kind):
    if kind == "one_pair_general":
        return _general_pair_row()
    if kind in ("good", "junk_row3"):
        return model.planted_rows(seed=23)
    if kind == "good2":
        return model.planted_rows(seed=25)
    if kind == "flat":
        return model.planted_rows(seed=24, flat=True)
    if kind == "pairs_eq_min":
        return model.planted_rows(seed=26, pairs=64)
    if kind == "pairs_below":
        return model.planted_rows(seed=26, pairs=63)
    if kind == "zero_g":
        row = model.planted_rows(seed=23).copy()
        row[model.G0:model.G0 + 6] = 0.0
        return row
    if kind == "step_345":
        return _diag_row(STEP_345)
    if kind == "near_pi":
        return _diag_row(np.concatenate([NEAR_PI, [0.1, -0.2, 0.3]]))
    if kind == "one_pair":
        return _one_pair_row()
    assert kind in ("nan_H", "nan_g", "nan_sw"), kind
    return model.planted_rows(seed=25)


NAN_AT = dict(nan_H=model.H0 + 7, nan_g=model.G0 + 2, nan_sw=model.SW)
EXACT_KINDS = ("step_345", "near_pi", "one_pair", "one_pair_general")        # the whole row goes into one group

# name -> (kinds, it, damping, threshold, min_pairs, status words the streams come in with)
T345 = float(np.linalg.norm(STEP_345))
SOLVE_SETTINGS = {
    "first":      (("good", "pairs_eq_min", "pairs_below", "nan_H", "nan_g", "nan_sw", "zero_g", "junk_row3", "flat", "good2"),
                   0, 1e-6, 1e-4, 64, (7, 1, 2, 4, 8, 0)),
    "threshold":  (("step_345", "one_pair", "near_pi", "good", "good2"), 0, 0.0, T345, 1, (0,)),
    "above":      (("step_345", "one_pair", "near_pi", "good", "good2"), 0, 0.0, float(np.nextafter(T345, 1.0)), 1, (0,)),
    "zero":       (("one_pair", "zero_g", "good", "step_345", "one_pair_general"), 0, 1e-6, 0.0, 1, (3,)),
    "later":      (("good", "good2", "junk_row3", "pairs_below", "flat"), 2, 1e-6, 1e-4, 64, (0, 1, 2, 4, 8, 0, 0)),
}


@functools.lru_cache(maxsize=None)
def solve_case(setting, S, G):
    """-> dict(partial (S, G, 32), rows (S, 32): the groups added in the kernel's order, T, T_clean (row 3 = 0 0 0 1: what
    the model takes), status (S,), kinds, and the launch's scalars)."""
    kinds, it, damping, threshold, min_pairs, words = SOLVE_SETTINGS[setting]
    r = np.random.default_rng([71, S, G, len(kinds), it])
    kind = [kinds[(s + G) % len(kinds)] for s in range(S)]
    partial = np.zeros((S, G, model.ROW))
    for s in range(S):
        row = _rows(kind[s])
        if kind[s] in EXACT_KINDS or G == 1:                  # the whole row in one group: zeros add back exactly
            partial[s, s % G] = row
        else:
            w = r.uniform(0.2, 1.0, (G, 1))
            partial[s] = row[None] * (w / w.sum())
            count = int(row[model.PAIRS])
            partial[s, :, model.PAIRS] = count // G
            partial[s, 0, model.PAIRS] += count % G
        if kind[s] in NAN_AT:
            partial[s, (s + 1) % G, NAN_AT[kind[s]]] = np.nan
    rows = np.zeros((S, model.ROW))
    with np.errstate(invalid="ignore"):
        for g in range(G):
            rows = rows + partial[:, g]
    clean = poses(r, S, 0.4)
    T = clean.copy()
    for s in range(S):
        if kind[s] == "junk_row3":
            T[s, 3] = JUNK_ROW3
    status = np.array([words[s % len(words)] for s in range(S)], dtype=np.int32)
    active = np.array([1 if (s % 3 != 1 and s != 32) else 0 for s in range(S)], dtype=np.int32)
    tol = np.array([solve_tolerance(kind[s], _rows(kind[s]), damping) for s in range(S)])
    return dict(setting=setting, S=S, G=G, kinds=kind, partial=partial, rows=rows, T=T, T_clean=clean, status=status, tol=tol,
                it=it, damping=damping, threshold=threshold, min_pairs=min_pairs, active=active)


def solve_expected(c, s, active=None):
    """The model's answer for stream s of a solve case; ``active``: the masked launch's words (looked at in iteration 0)."""
    if active is not None and c["it"] == 0 and not active[s]:
        return dict(delta=np.zeros((6,)), T=c["T_clean"][s].copy(), status=IDLE, moved=False, idle=True)
    out = model.solve(c["rows"][s], c["T_clean"][s], int(c["status"][s]), c["it"], c["damping"], c["threshold"], c["min_pairs"])
    out["idle"] = False
    return out


# ---- begin, push, gated push --------------------------------------------------------------------------------------------------------

PUSH_N = (64, 65, 127, 128)
PUSH_M = (1, 4, 64)
BLOCK_BYTES = 64 * 16 + 32


def ws_blocks(n):
    """Blocks of a cloud's search structure for 64 <= n <= 960: ceil(n / 64) blocks of points and two slabs."""
    assert 64 <= n <= 960
    return (n + 63) // 64 + 2


def mul_rows(A, T):
    """se3_mul in its order, over the slots: A (M, 4, 4), T (4, 4) -> rows 0..2 of A[m] T, (M, 3, 4)."""
    out = np.empty((A.shape[0], 3, 4))
    for i in range(3):
        for j in range(4):
            s = (A[:, i, 0] * T[0, j] + A[:, i, 1] * T[1, j]) + A[:, i, 2] * T[2, j]
            out[:, i, j] = s + A[:, i, 3] if j == 3 else s
    return out


def rebase_rotations(T, R):
    """Rm <- R_T^T Rm in icp_slot_after_push's order: R (M, 3, 3)."""
    out = np.empty_like(R)
    for i in range(3):
        for j in range(3):
            out[:, i, j] = (T[0, i] * R[:, 0, j] + T[1, i] * R[:, 1, j]) + T[2, i] * R[:, 2, j]
    return out


class Maps:
    """icp_model.Map's rules for S streams, with the device's words (active, restart / armed, insert), its clamp of the
    cursor and its order of operations, so that every array is the device's bit for bit.  ws_rows (S, M, nblk * 1024) and
    ws_boxes (S, M, nblk * 32) bytes are the two sections of the maps' search structures."""

    def __init__(self, S, M, n, seed):
        r = np.random.default_rng([83, S, M, n, seed])
        nblk = ws_blocks(n)
        self.S, self.M, self.n, self.nblk = S, M, n, nblk
        self.xyz = r.uniform(-9.0, 9.0, (S, M, n, 3)).astype(F)
        self.normals = r.uniform(-1.0, 1.0, (S, M, n, 3)).astype(F)
        self.ws_rows = r.integers(0, 256, (S, M, nblk * 1024), dtype=np.uint8)
        self.ws_boxes = r.integers(0, 256, (S, M, nblk * 32), dtype=np.uint8)
        self.A = poses(r, S * M).reshape(S, M, 4, 4)
        self.A[:, M // 2, 3] = (0.25, -3.0, 1e30, 7.0)                  # a row 3 that a re-base must leave alone
        self.R = np.ascontiguousarray(np.transpose(poses(r, S * M)[:, :3, :3].reshape(S, M, 3, 3), (0, 1, 3, 2)))
        self.live = r.integers(0, 2, (S, M)).astype(np.int32)
        self.cursor = r.integers(0, M, (S,)).astype(np.int32)

    def ws(self):
        return np.concatenate([self.ws_rows.reshape(-1), self.ws_boxes.reshape(-1)])

    def state(self):
        return dict(map_xyz=self.xyz, map_normals=self.normals, map_ws=self.ws(), A=self.A, R=self.R, live=self.live,
                    cursor=self.cursor)

    def begin(self, active, restart, armed=None):
        for s in range(self.S):
            if active[s] and (restart[s] or (armed is not None and armed[s])):
                self.A[s], self.R[s], self.live[s], self.cursor[s] = np.eye(4), np.eye(3), 0, 0
                if armed is not None:
                    armed[s] = 0

    def push(self, T, frame, active=None, insert=None):
        """frame: dict(cloud (S, n, 3), normals (S, n, 3), ws_rows (S, nblk * 1024), ws_boxes (S, nblk * 32))."""
        for s in range(self.S):
            if active is not None and not active[s]:
                continue
            ins = insert is None or bool(insert[s])
            slot = min(max(int(self.cursor[s]), 0), self.M - 1)
            moved, turned = mul_rows(self.A[s], T[s]), rebase_rotations(T[s], self.R[s])
            for m in range(self.M):
                if ins and m == slot:
                    self.A[s, m], self.R[s, m], self.live[s, m] = np.eye(4), np.eye(3), 1
                elif self.live[s, m]:
                    self.A[s, m, :3], self.R[s, m] = moved[m], turned[m]
            if ins:
                self.xyz[s, slot], self.normals[s, slot] = frame["cloud"][s], frame["normals"][s]
                self.ws_rows[s, slot], self.ws_boxes[s, slot] = frame["ws_rows"][s], frame["ws_boxes"][s]
                self.cursor[s] = 0 if slot + 1 == self.M else slot + 1


def frame(S, n, seed):
    """A staged frame with planted bytes for its structure: the push copies, it does not search."""
    r = np.random.default_rng([89, S, n, seed])
    nblk = ws_blocks(n)
    f = dict(cloud=r.uniform(-9.0, 9.0, (S, n, 3)).astype(F), normals=r.uniform(-1.0, 1.0, (S, n, 3)).astype(F),
             ws_rows=r.integers(0, 256, (S, nblk * 1024), dtype=np.uint8), ws_boxes=r.integers(0, 256, (S, nblk * 32), dtype=np.uint8),
             T=poses(r, S, 0.2, 0.5))
    f["T"][:, 3] = (9.0, np.nan, -1e30, 0.5)                            # the pose's row 3 is never read
    f["stage_ws"] = np.concatenate([f["ws_rows"].reshape(-1), f["ws_boxes"].reshape(-1)])
    return f


def words(k, S=3):
    """Every joint setting of k 0 / 1 words per stream across S streams -> a list of (S, k) int32 arrays."""
    return [np.array(w, dtype=np.int32).reshape(S, k) for w in itertools.product((0, 1), repeat=S * k)]
