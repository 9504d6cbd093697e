"""The case tables of tests/test_gpu_gather_forward.py, with their inputs and host references, shared with
tests/test_gather_plan_cpu.py, which proves through group_points_plan_query that the group rows reach every form
gp_forward (csrc/group_points.hip) can launch and hold both sides of every size threshold.

The forward index-driven kernels copy or combine SOURCE ELEMENTS: out[b, c, j, t] = points[b, c, idx[b, j, t]] and its
relatives.  Everything here is CPU numpy / torch and every comparison is exact, on the int32 view of the fp32 bits.

A group form is (kernel, T, NT, staged_vec, passes, tail):
  kernel      "direct_scalar" (P % 4 != 0 or an unaligned pointer), "direct_vec4" (LDS off, or min(c, 8) rows of n floats
              beyond 128 KiB) or "lds" (group_points_lds_kernel<T, NT>);
  T, NT       threads of a workgroup (1024 / 512 / 256) and non-temporal stores; direct kernels: 256, 0;
  staged_vec  LDS rows staged with 16-byte copies (n % 4 == 0); direct kernels: 0;
  passes      of a workgroup's ``p += 4 T`` loop: "one", "several", or "several_short" (several, the last with fewer than
              4 T positions); direct kernels: "one";
  tail        c % 8 != 0: the last channel slice is narrower.
Options: short_wg (the last workgroup covers fewer than per_wg positions), misalign (idx starts 4 bytes into a buffer:
P % 4 == 0 must still take the scalar kernel), side (where min(c, 8) * n * 4 lies against 64 and 128 KiB).

Two fills go through every copying kernel (group_points, gather_points, broadcast_centre, channels 0..5 of
geometry_encode): "identity", points[b, c, i] = ((b * C) + c) * n + i as an exact fp32 integer (< 2^24), so a wrong source
element, channel or cloud is an exact mismatch that names the culprit; and "bits", random 32-bit words with -0.0, both
infinities, subnormals and quiet / signalling NaNs with payloads planted at the elements every index list reads.  The
arithmetic outputs (xyz_diff, channels 6..9 of geometry_encode, three_interpolate) get finite, normal inputs only: their
references are numpy float32 operations, one rounding per operation, in the order the kernel's comment states, and IEEE
leaves the payload of a NaN result open.
"""
from collections import namedtuple

import numpy as np
import torch

KIB = 1024
SENTINEL = np.int32(0x7FC5A5A5)         # a NaN with a payload: what every channel around a written slice must still hold
SPECIALS = np.array([0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x7FC12345, 0xFFC00001, 0x7F812345,
                     0x00000000, 0xFFBFFFFF], dtype=np.uint32).view(np.int32)
NEG_ZERO, NEG_NAN_PAYLOAD = np.array([0x80000000, 0xFFC12345], dtype=np.uint32).view(np.int32)

Group = namedtuple("Group", "b c n s k tune want opts")
Gather = namedtuple("Gather", "b c n m")
Interp = namedtuple("Interp", "b c m n")          # m coarse points interpolated to n fine ones
Bcast = namedtuple("Bcast", "b c s k c_off")
Geo = namedtuple("Geo", "b n s k")
ThreeNN = namedtuple("ThreeNN", "b n m")          # n unknown points, m known ones
Ball = namedtuple("Ball", "b n m nsample")        # n candidates, m queries

DEFAULT_TUNE = dict(use_lds=1, threads=0, target=0, nt=1)      # what the launcher uses with nothing set
PASSES = ("one", "several", "several_short")


def _g(b, c, n, s, k, want, **kw):
    tune = dict(DEFAULT_TUNE)
    for key in list(kw):
        if key in tune:
            tune[key] = kw.pop(key)
    return Group(b, c, n, s, k, tune, want, kw)


def _lds_rows():
    rows = []
    for T in (1024, 512, 256):
        for nt in (1, 0):
            for staged in (1, 0):
                n = 64 if staged else 63
                for tail in (False, True):
                    c = 9 if tail else 8
                    # one pass (a full one with the 16-byte staging, a short one with the scalar staging), two full
                    # passes, two full passes and a third of 4 positions; target = 1: one workgroup per slice
                    for passes, P, b in (("one", 4 * T if staged else 4 * T - 12, 2), ("several", 8 * T, 1),
                                         ("several_short", 8 * T + 4, 1)):
                        rows.append(_g(b, c, n, P // 4, 4, ("lds", T, nt, staged, passes, tail), threads=T, nt=nt, target=1))
        for staged in (1, 0):
            # c = 9: two slices; target = 4 asks for two workgroups per slice: 8 T positions, then a workgroup of 4
            rows.append(_g(1, 9, 64 if staged else 63, 2 * T + 1, 4, ("lds", T, staged, staged, "several", True),
                           threads=T, nt=staged, target=4, short_wg=True))
        for nt in (1, 0):
            # 128 KiB of rows: this instantiation's hipFuncSetAttribute call
            rows.append(_g(1, 9, 4096, T + 1, 4, ("lds", T, nt, 1, "several_short", True), threads=T, nt=nt, target=1,
                           side="=128K"))
    return rows


def _direct_rows():
    rows = []
    for c in (1, 7, 8, 9):
        tail = c % 8 != 0
        want = ("direct_scalar", 256, 0, 0, "one", tail)
        rows += [_g(2, c, 50, 85, 3, want), _g(2, c, 50, 257, 1, want), _g(1, c, 50, 64, 4, want, misalign=True)]
    for c in (8, 3, 9):
        want = ("direct_vec4", 256, 0, 0, "one", c % 8 != 0)
        # LDS switched off at a small n: a few positions, one full 1024-position block, two blocks (the second: one thread)
        rows += [_g(2, c, 64, 3, 4, want, use_lds=0), _g(1, c, 63, 256, 4, want, use_lds=0), _g(2, c, 64, 257, 4, want, use_lds=0)]
    return rows


THRESHOLD_P = 257 * 1024      # more than 256 workgroups of 256 threads: where the 512 | 256 workgroup target shows in the grid


def _threshold_rows():
    lds = lambda staged, tail, passes="one": ("lds", 1024, 1, staged, passes, tail)
    return [
        # 128 KiB: the last n whose min(c, 8) rows fit, and one more -> the direct kernel
        _g(1, 8, 4096, 64, 4, lds(1, False), side="=128K"), _g(1, 8, 4097, 64, 4, ("direct_vec4", 256, 0, 0, "one", False), side=">128K"),
        _g(1, 9, 4096, 64, 4, lds(1, True), side="=128K"), _g(1, 9, 4097, 64, 4, ("direct_vec4", 256, 0, 0, "one", True), side=">128K"),
        _g(1, 3, 10922, 16, 4, lds(0, True), side=">64K"), _g(1, 3, 10923, 16, 4, ("direct_vec4", 256, 0, 0, "one", True), side=">128K"),
        # 64 KiB: below it the launcher aims for 512 workgroups, from it on for 256 (seen in the grid from 257 workgroups
        # of 256 threads on); above it the kernel needs its dynamic LDS limit raised
        _g(1, 8, 2044, THRESHOLD_P // 4, 4, ("lds", 256, 1, 1, "one", False), threads=256, side="<64K", gx=257),
        _g(1, 8, 2048, THRESHOLD_P // 4, 4, ("lds", 256, 1, 1, "several", False), threads=256, side="=64K", gx=129, short_wg=True),
        _g(2, 16, 2044, 37, 4, lds(1, False), side="<64K"), _g(2, 16, 2048, 37, 4, lds(1, False), side="=64K"),
        _g(2, 16, 2052, 37, 4, lds(1, False), side=">64K"),
        # the network's level-0 grouping of coordinates: 3 rows of 8192 floats = 96 KiB
        _g(2, 3, 8192, 64, 32, lds(1, True), side=">64K"),
    ]


GROUP_CASES = _direct_rows() + _lds_rows() + _threshold_rows()

# (n, n + 1) pairs that the table must hold with c >= 8 and with c = 3: the kernel changes between them
SIZE_THRESHOLDS = ((8, 4096), (3, 10922))
LDS_64K_ROWS = (2044, 2048, 2052)          # c >= 8: lds_bytes below, at and above 64 KiB

GATHER_CASES = [Gather(2, c, 100 + m, m) for m in (1, 255, 256, 257) for c in (1, 8, 9)]
INTERP_CASES = [Interp(2, c, 64 + n % 7, n) for n in (1, 255, 256, 257) for c in (1, 8, 9)]
# P = s * k: k = 1, 3, 5 make the four positions of a thread straddle centres; P % 4 in {0, 1, 2, 3}; more than one block of
# 1024 positions; odd P at an odd channel offset: rows that start 4, 8 and 12 bytes off the 16-byte grid
BCAST_CASES = [Bcast(2, 5, 256, 1, 1), Bcast(2, 5, 257, 1, 1), Bcast(2, 5, 84, 3, 1), Bcast(2, 5, 85, 3, 1), Bcast(2, 5, 86, 3, 2),
               Bcast(2, 5, 64, 4, 1), Bcast(2, 5, 300, 4, 3), Bcast(2, 5, 51, 5, 1), Bcast(2, 5, 52, 5, 2), Bcast(2, 5, 205, 5, 1),
               Bcast(2, 5, 345, 3, 1), Bcast(2, 5, 9, 32, 1), Bcast(2, 5, 33, 32, 1), Bcast(1, 9, 1, 1, 1), Bcast(1, 3, 1, 3, 0)]
GEO_CASES = [Geo(2, 300, 255, 1), Geo(2, 300, 256, 1), Geo(2, 300, 257, 1), Geo(2, 300, 85, 3), Geo(2, 300, 86, 3),
             Geo(2, 300, 8, 32), Geo(2, 300, 9, 32), Geo(1, 40, 1, 3)]

THREE_NN_CASES = [ThreeNN(2, n, m) for m in (1, 2, 3, 63, 64, 65, 129, 200) for n in (1, 3, 4, 5)]
BALL_CASES = [Ball(2, n, 6, ns) for n in (1, 63, 64, 65, 200) for ns in (1, 5, 64, 70)]
BALL_RADIUS = 2.0                         # r * r = 4 exactly: lattice points at distance 2 sit on the sphere


def case_id(c):
    parts = [type(c).__name__.lower()] + [str(v) for v in c if isinstance(v, int)]
    if isinstance(c, Group):
        parts += ["%s%d" % (k[:2], v) for k, v in sorted(c.tune.items()) if v != DEFAULT_TUNE[k]] + sorted(
            k for k, v in c.opts.items() if v is True)
    return "-".join(parts)


def _seed(c, salt=0):
    return (sum((i + 1) * 7919 * v for i, v in enumerate(v for v in c if isinstance(v, int))) + 104729 * salt) % (2 ** 31)


# ---- group_points: forms ------------------------------------------------------------------------------------------------
def lds_need(c, n):
    return min(c, 8) * n * 4


def side(c, n):
    need = lds_need(c, n)
    for name, ok in (("<64K", need < 64 * KIB), ("=64K", need == 64 * KIB), (">64K", 64 * KIB < need < 128 * KIB),
                     ("=128K", need == 128 * KIB), (">128K", need > 128 * KIB)):
        if ok:
            return name


def workgroup_lengths(plan, P):
    return [min(plan["per_wg"], P - w * plan["per_wg"]) for w in range(plan["gx"])]


def group_form(plan, P):
    """The form of a ``_ext.group_points_plan`` answer for P positions."""
    if plan["form"] != "lds":
        passes = "one"
    else:
        step = 4 * plan["T"]
        several = [L for L in workgroup_lengths(plan, P) if L > step]
        passes = "one" if not several else ("several_short" if any(L % step for L in several) else "several")
    return (plan["form"], plan["T"], plan["nt"], plan["staged_vec"], passes, plan["tail"] != 0)


def short_last_workgroup(plan, P):
    lens = workgroup_lengths(plan, P)
    return plan["form"] == "lds" and len(lens) > 1 and 0 < lens[-1] < plan["per_wg"]


def plan_of(E, case, **override):
    tune = dict(case.tune, **override)
    return E.group_points_plan(case.b, case.c, case.n, case.s * case.k, aligned=not case.opts.get("misalign", False), **tune)


# ---- fills --------------------------------------------------------------------------------------------------------------
def fill_identity(b, c, n):
    """(b, c, n) int32 bits of the fp32 integers ((b * C) + c) * n + i."""
    assert b * c * n < 2 ** 24
    return np.arange(b * c * n, dtype=np.float32).reshape(b, c, n).view(np.int32)


def fill_bits(b, c, n, seed):
    """(b, c, n) random int32 words; every fourth element one of SPECIALS, element 0 of every row -0.0 and element n - 1 a
    negative NaN with a payload (n == 1: the NaN)."""
    rng = np.random.default_rng(seed)
    w = rng.integers(-2 ** 31, 2 ** 31, size=(b, c, n), dtype=np.int64).astype(np.int32)
    flat = w.reshape(-1)
    at = np.arange(1, flat.size, 4)
    flat[at] = SPECIALS[(at // 4) % len(SPECIALS)]
    w[:, :, 0] = NEG_ZERO
    w[:, :, n - 1] = NEG_NAN_PAYLOAD
    return w


FILLS = ("identity", "bits")


def fill(kind, b, c, n, seed):
    return fill_identity(b, c, n) if kind == "identity" else fill_bits(b, c, n, seed)


def as_f32(bits):
    """int32 numpy words -> fp32 torch tensor of the same bits."""
    return torch.from_numpy(np.ascontiguousarray(bits)).view(torch.float32)


def bits_of(t):
    """fp32 torch tensor (any device) -> int32 numpy words."""
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def index_list(b, P, n, seed, rows=None):
    """(b, P) int32 in [0, n): random, n - 1 at the first position and 0 at the last, and with ``rows`` = (s, k) the
    middle row all equal."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n, size=(b, P), dtype=np.int64).astype(np.int32)
    if rows is not None and rows[0] >= 3:
        s, k = rows
        idx.reshape(b, s, k)[:, s // 2, :] = (n // 2 + np.arange(b, dtype=np.int32))[:, None] % n
    if P >= 2:
        idx[:, 0] = n - 1
        idx[:, P - 1] = 0
    return idx


def group_inputs(case, kind):
    """-> (points bits (b, c, n), idx (b, s, k))."""
    assert case.s >= 3
    idx = index_list(case.b, case.s * case.k, case.n, _seed(case), (case.s, case.k)).reshape(case.b, case.s, case.k)
    return fill(kind, case.b, case.c, case.n, _seed(case, 1)), idx


def ref_group(bits, idx):
    """out[b, c, j, t] = points[b, c, idx[b, j, t]] on the int32 view."""
    b, c, n = bits.shape
    return bits[np.arange(b)[:, None, None, None], np.arange(c)[None, :, None, None], idx[:, None].astype(np.intp)]


def stack_of(b, ctot, s, k):
    return np.full((b, ctot, s, k), SENTINEL, dtype=np.int32)


def ref_stack(part, c_off, after):
    """The (b, c_off + c + after, s, k) stack a ``*_into`` call must leave: the part in its slice, sentinels around it."""
    b, c, s, k = part.shape
    st = stack_of(b, c_off + c + after, s, k)
    st[:, c_off:c_off + c] = part
    return st


# ---- gather_points, three_interpolate -------------------------------------------------------------------------------------
def gather_inputs(case, kind):
    idx = index_list(case.b, case.m, case.n, _seed(case))
    return fill(kind, case.b, case.c, case.n, _seed(case, 1)), idx


def ref_gather(bits, idx):
    b, c, n = bits.shape
    return bits[np.arange(b)[:, None, None], np.arange(c)[None, :, None], idx[:, None].astype(np.intp)]


def _normal_f32(rng, shape, scale=8.0):
    """Finite, normal fp32 values of magnitude in [2^-6, scale) with both signs."""
    v = (rng.uniform(2.0 ** -6, scale, size=shape) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)
    assert np.isfinite(v).all() and (np.abs(v) >= np.finfo(np.float32).tiny).all()
    return v


def interp_inputs(case):
    """-> (points (b, c, m) f32, idx (b, n, 3) i32, weight (b, n, 3) f32): weights in (0, 1), with exact 0 and 1 in the
    rows j % 5 == 0 (one neighbour takes everything, each position in turn)."""
    rng = np.random.default_rng(_seed(case))
    pts = _normal_f32(rng, (case.b, case.c, case.m))
    idx = index_list(case.b, case.n * 3, case.m, _seed(case, 1)).reshape(case.b, case.n, 3)
    w = rng.uniform(2.0 ** -6, 1.0, size=(case.b, case.n, 3)).astype(np.float32)
    for j in range(0, case.n, 5):
        w[:, j] = np.eye(3, dtype=np.float32)[(j // 5) % 3]
    return pts, idx, w


def ref_interp(pts, idx, w):
    """(p[i1] * w1 + p[i2] * w2) + p[i3] * w3 in fp32, one rounding per operation (csrc/interpolate.hip)."""
    b, c, m = pts.shape
    g = pts[np.arange(b)[:, None, None, None], np.arange(c)[None, :, None, None], idx[:, None].astype(np.intp)]   # (b, c, n, 3)
    prod = g * w[:, None]
    assert prod.dtype == np.float32
    return (prod[..., 0] + prod[..., 1]) + prod[..., 2]


# ---- the parts of the concatenated stack input ----------------------------------------------------------------------------
def bcast_inputs(case, kind):
    return fill(kind, case.b, case.c, case.s, _seed(case, 1))


def ref_bcast(bits, k, shift=0):
    """out[b, c, j, t] = feats[b, c, j].  ``shift``: the planted fault j = (p + shift) / k."""
    b, c, s = bits.shape
    j = np.minimum((np.arange(s * k) + shift) // k, s - 1)
    return bits[:, :, j].reshape(b, c, s, k)


def geo_inputs(case, kind):
    """-> (centre bits (b, 3, s), src bits (b, 3, n), idx (b, s, k)); the centres are the first s sources and every centre is
    its own first neighbour.  kind "real": finite normal coordinates for the arithmetic channels."""
    b, n, s, k = case
    assert n >= s
    if kind == "real":
        rng = np.random.default_rng(_seed(case, 2))
        src = _normal_f32(rng, (b, 3, n), 16.0).view(np.int32)
    else:
        src = fill(kind, b, 3, n, _seed(case, 1))
    idx = index_list(b, s * k, n, _seed(case), (s, k)).reshape(b, s, k)
    idx[:, :, 0] = np.arange(s, dtype=np.int32)
    return np.ascontiguousarray(src[:, :, :s]), src, idx


def ref_geo_copies(centre, src, idx, shift=0):
    """Channels 0..5 of geometry_encode on the int32 view: the centre tiled over its k neighbours, the gathered neighbour."""
    k = idx.shape[2]
    return np.concatenate((ref_bcast(centre, k, shift), ref_group(src, idx)), axis=1)


def ref_xyz_diff(centre, src, idx):
    """q - p in fp32 (inputs as int32 bits of finite values) -> (b, 3, s, k) f32."""
    p = ref_bcast(centre, idx.shape[2]).view(np.float32)
    q = ref_group(src, idx).view(np.float32)
    return q - p


def ref_geo(centre, src, idx):
    """All 10 channels as int32 bits: [p, q, q - p, sqrt(((dx dx + dy dy) + dz dz) + 1e-20f)], each product and sum rounded to
    fp32, the square root of that fp32 value taken in double and rounded once (exact for fp32)."""
    d = ref_xyz_diff(centre, src, idx)
    sq = d * d
    ssum = ((sq[:, 0] + sq[:, 1]) + sq[:, 2]) + np.float32(1e-20)
    assert sq.dtype == np.float32 and ssum.dtype == np.float32
    e = np.sqrt(ssum.astype(np.float64)).astype(np.float32)
    return np.concatenate((ref_geo_copies(centre, src, idx), d.view(np.int32), e[:, None].view(np.int32)), axis=1)


# ---- search rows ----------------------------------------------------------------------------------------------------------
NN_SAME_LANE, NN_NEXT_LANE = 5, 20       # duplicates of a marked point at k, k + 64 (, k + 128) and at k, k + 1
NN_MARK_A, NN_MARK_B = (7.0, -7.0, 7.0), (-7.0, 7.0, 7.0)


def three_nn_inputs(case):
    """-> (unknown (b, n, 3), known (b, m, 3)) on the integer lattice [-2, 2]^3 (125 places: ties are the rule); unknown 0 is
    the marked point A, copies of which sit at known NN_SAME_LANE + 64 i (one lane of the wave), unknown 1 is B with
    copies at known NN_NEXT_LANE, + 1 (neighbouring lanes) -- where m reaches them."""
    b, n, m = case
    rng = np.random.default_rng(_seed(case))
    known = rng.integers(-2, 3, size=(b, m, 3)).astype(np.float32)
    unknown = rng.integers(-2, 3, size=(b, n, 3)).astype(np.float32)
    for i in range(NN_SAME_LANE, m, 64):
        known[:, i] = NN_MARK_A
    for i in (NN_NEXT_LANE, NN_NEXT_LANE + 1):
        if i < m:
            known[:, i] = NN_MARK_B
    unknown[:, 0] = NN_MARK_A
    if n > 1:
        unknown[:, 1] = NN_MARK_B
    return unknown, known


# cloud 0 of every ball_query row, by candidate index (where n reaches it): hits and on-the-sphere points of three queries
BALL_ORIGINS = ((0.0, 0.0, 0.0), (0.0, 1000.0, 0.0), (0.0, 0.0, 1000.0))     # query 0, 1, 2; query 2 has no hit at all
BALL_Q0_HITS = (2, 10, 50) + tuple(i for i in range(64, 76) if i != 70)      # 3 in the first step, 11 in the second
BALL_Q0_ON_SPHERE = (0, 5, 70)                                             # d2 == r * r exactly: not hits
BALL_Q1_HITS = (130, 150)                                                  # the first hit lies in the third step
_OFFSETS = np.array([(1, 0, 0), (0, 1, 0), (1, 1, 1), (0, 0, 0), (-1, 1, 0), (0, -1, -1), (1, -1, 1)], dtype=np.float32)


def ball_inputs(case):
    """-> (new_xyz (b, m, 3), xyz (b, n, 3)).  Cloud 0: every candidate far from every query except the indices above;
    cloud 1: candidates and queries on the lattice [-2, 2]^3, where d2 == 4 is frequent."""
    b, n, m, _ = case
    assert b == 2 and m >= 4
    rng = np.random.default_rng(_seed(case))
    xyz = rng.integers(-2, 3, size=(b, n, 3)).astype(np.float32)
    q = rng.integers(-2, 3, size=(b, m, 3)).astype(np.float32)
    xyz[0] = np.stack((100.0 + np.arange(n), np.zeros(n), np.zeros(n)), axis=1)
    q[0, :3] = BALL_ORIGINS
    q[0, 3:] = BALL_ORIGINS[0]
    q[0, 3:, 0] = 1.0                              # queries next to query 0: other hit lists over the same candidates
    for t, i in enumerate(BALL_Q0_HITS):
        if i < n:
            xyz[0, i] = np.array(BALL_ORIGINS[0], dtype=np.float32) + _OFFSETS[t % len(_OFFSETS)]
    for t, i in enumerate(BALL_Q0_ON_SPHERE):
        if i < n:
            xyz[0, i] = np.array(BALL_ORIGINS[0], dtype=np.float32) + np.roll(np.array([2.0, 0.0, 0.0], dtype=np.float32), t)
    for t, i in enumerate(BALL_Q1_HITS):
        if i < n:
            xyz[0, i] = np.array(BALL_ORIGINS[1], dtype=np.float32) + _OFFSETS[t]
    return q, xyz
