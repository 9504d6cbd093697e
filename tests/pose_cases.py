"""Cases and host models for the kernels that turn the network's last tensor into the pose: ``pose_head_kernel`` and
``masked_pool_kernel`` (csrc/fused_layers.hip) and ``quat_warp_kernel<false/true>`` (csrc/warp.hip).  Host only: numpy
and torch on the CPU, no GPU.  tests/test_pose_cases_cpu.py shows that the cases tell a correct implementation from the
wrong ones in ``HEAD_MUTANTS`` / ``WARP_MUTANTS``; tests/test_gpu_pose_path.py runs the kernels on the same cases.

Two host models:

* ``warp_expr``: PW/PWCLO_utils.py:31-63 component by component in the kernel's (= the reference's) left-to-right order,
  every product and sum one rounded operation of ``dtype``.  In float32 it is what the kernels promise bit for bit, in
  float64 the exact value.
* ``head_model``: PW/pose_calculator.py:47-86 in eval mode, the composition of PW/pose_warp_refinement.py:139,148 and the
  row of PW/pwclo_net.py:195-205, as oracle/model.py states them.  In float64 the exact value, in float32 the source of
  E32 (tests/stack_reference.py: fp32_figures); ``order="slots"`` is float32 with the pooling summed the way the kernel
  sums it (64 partial sums over points i = slot mod 64, combined one after the other).
"""
import functools
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import params

PREFIX = "pose_calculator_4"
B_HEAD = 8          # clouds per head case: q has 32 numbers, t 24, the row 56
SLOTS = 64          # (wave, sub) point slots of pose_head_kernel's pooling


# ---- the warp ------------------------------------------------------------------------------------------------------------

def _hamilton(a, b, contract=None):
    """a (x) b, components in the order of csrc/warp.hip: hamilton().  ``contract`` = index of one component that is
    computed in float64 and rounded once instead: what a chain of fused multiply-adds looks like."""
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    expr = (lambda aw, ax, ay, az, bw, bx, by, bz: ((aw * bw - ax * bx) - ay * by) - az * bz,
            lambda aw, ax, ay, az, bw, bx, by, bz: ((aw * bx + ax * bw) + ay * bz) - az * by,
            lambda aw, ax, ay, az, bw, bx, by, bz: ((aw * by - ax * bz) + ay * bw) + az * bx,
            lambda aw, ax, ay, az, bw, bx, by, bz: ((aw * bz + ax * by) - ay * bx) + az * bw)
    out = []
    for i, f in enumerate(expr):
        if i == contract:
            wide = [np.asarray(v, dtype=np.float64) for v in (aw, ax, ay, az, bw, bx, by, bz)]
            out.append(f(*wide).astype(np.asarray(aw).dtype))
        else:
            out.append(f(aw, ax, ay, az, bw, bx, by, bz))
    return out


def _warp_components(q, p, t, eps, mutant=None):
    """q = (w, x, y, z), p = (px, py, pz), t = (tx, ty, tz): arrays (numpy or torch) that broadcast against each other,
    all of one dtype; eps = 1e-10 in that dtype.  -> (x', y', z')."""
    w, x, y, z = q
    q2 = (((w * w + x * x) + y * y) + z * z) + eps
    if mutant == "conjugate_not_divided":
        qi = (w, x * -1, y * -1, z * -1)
    else:
        qi = (w / q2, (x * -1) / q2, (y * -1) / q2, (z * -1) / q2)
    zero = p[0] - p[0]                            # (0, p): +0.0 like the kernel's literal, for every finite coordinate
    r1 = _hamilton(q, (zero, p[0], p[1], p[2]))
    r = _hamilton(r1, qi, contract=1 if mutant == "contracted_component" else None)
    return r[1] + t[0], r[2] + t[1], r[3] + t[2]


def warp_expr(xyz, q, t, point_major, dtype=np.float32, mutant=None):
    """xyz (B,N,3) if ``point_major`` else (B,3,N); q (B,4); t (B,3) -> the warped cloud in xyz's layout, a numpy array
    of ``dtype``.  No np.sum / torch.sum anywhere: their order over four elements is not defined."""
    xyz, q, t = (np.asarray(v.detach().cpu() if torch.is_tensor(v) else v).astype(dtype) for v in (xyz, q, t))
    B = xyz.shape[0]
    q, t = q.reshape(B, 4), t.reshape(B, 3)
    p = [xyz[:, :, i] if point_major else xyz[:, i, :] for i in range(3)]
    with np.errstate(all="ignore"):
        out = _warp_components([q[:, i:i + 1] for i in range(4)], p, [t[:, i:i + 1] for i in range(3)],
                               dtype(1e-10), mutant)
    return np.stack(out, axis=2 if point_major else 1).astype(dtype)


WARP_MUTANTS = ("conjugate_not_divided", "contracted_component")

# every case runs through both layouts: the point-major and the channel-major kernel see the same cloud
WarpCase = namedtuple("WarpCase", "name B n q_form seed why")
Q_FORMS = ("unit", "x1.7", "x1e-6", "zero")


def _warp_cases():
    whys = {1: "a single point: one thread of one block works", 255: "one short of the 256-thread block",
            256: "exactly one block", 257: "one point into the second block",
            2049: "nine blocks, the last with one point; the product's level-2 size plus one"}
    cases = []
    for i, n in enumerate((1, 255, 256, 257, 2049)):      # every size with every q form; B alternates, so every size and
        for j, form in enumerate(Q_FORMS):                # every form meets both batch sizes
            B = 1 if (i + j) % 2 == 0 else 3
            cases.append(WarpCase("n%d_b%d_%s" % (n, B, form), B, n, form, 500 + len(cases), whys[n]))
    return cases


WARP_CASES = _warp_cases()
WARP_BY_NAME = {c.name: c for c in WARP_CASES}


def warp_inputs(case):
    """-> xyz (B,n,3) point-major, q (B,4), t (B,3): float32 CPU tensors.  Points uniform in +-30 with a few rows set to 0
    and to +-1e4; q by ``case.q_form``: unit; unit x 1.7; unit x 1e-6 (|q|^2 = 1e-12, below the 1e-10 it is added to);
    exactly zero (the result is t)."""
    g = torch.Generator().manual_seed(case.seed)
    xyz = (torch.rand(case.B, case.n, 3, generator=g) * 2 - 1) * 30
    for j, val in ((0, 0.0), (3, 1e4), (7, -1e4)):
        if j < case.n:
            xyz[:, j] = val
    if case.n > 11:
        xyz[:, 11] = torch.tensor([1e4, 0.0, -1e4])
    q = F.normalize(torch.randn(case.B, 4, generator=g), dim=1)
    q = q * {"unit": 1.0, "x1.7": 1.7, "x1e-6": 1e-6, "zero": 0.0}[case.q_form]
    t = torch.randn(case.B, 3, generator=g)
    return xyz.contiguous(), q.contiguous(), t.contiguous()


# ---- the eval pose head --------------------------------------------------------------------------------------------------

HeadCase = namedtuple("HeadCase", "name N spread prev warp_n level seed why")
# spread: "randn3" = randn * 3; "u80" / "u100" = uniform over +-80 / +-100.  prev: None = level-4 form (no coarse pose), or
# the factor on a unit q_prev.  warp_n: 0 = no in-launch warp.  level: the row of pose_params (B,4,7) that is written.
# Seeds: a correct float32 head in the kernel's summation order must sit at half the criterion's bound or below (both ratios
# to E32 <= 2, tests/test_pose_cases_cpu.py); the ratio is a maximum over a few hundred numbers and scatters from seed to
# seed (around N = 64 the RMS ratio of the pooled features is close to 2 whatever the seed: 64 terms added one after the
# other against torch's blocked sum), so each seed is the best of 16 tried for that condition.  The criterion is never touched.
# +-80 does not overflow float32 without the maximum subtraction (e^80 x 256 = 1.4e37): it guards the range just below
# the overflow; the "u100" row is the one that a soft-max without the subtraction cannot pass.
HEAD_CASES = [
    HeadCase("n1", 1, "randn3", None, 0, 3, 11, "one point: 63 of 64 slots stay empty, soft-max is exactly 1"),
    HeadCase("n1_prev_w1", 1, "randn3", 1.0, 1, 2, 12, "one point, composed, one warped point: one thread of 1024 warps"),
    HeadCase("n3_prev1.7_w777", 3, "randn3", 1.7, 777, 0, 1513, "fewer points than slots; row normalisation divides by 1.7"),
    HeadCase("n63_w1023", 63, "randn3", None, 1023, 3, 514, "one slot empty; warp one short of the workgroup"),
    HeadCase("n64_prev_w1024", 64, "randn3", 1.0, 1024, 1, 915, "exactly one trip; warp of exactly one trip"),
    HeadCase("n65_w1025", 65, "randn3", None, 1025, 3, 1416, "one point into the second trip; warp's second trip, no q_prev"),
    HeadCase("n65_u80_prev", 65, "u80", 1.0, 0, 2, 1417, "logits over +-80 with a partial trip"),
    HeadCase("n255_prev0.3_w1023", 255, "randn3", 0.3, 1023, 0, 318, "one short of the 4 x 64 unroll; row normalisation divides by 0.3"),
    HeadCase("n256_w2049", 256, "randn3", None, 2049, 3, 519, "exactly the unroll; warp of three trips, no q_prev"),
    HeadCase("n256_u80_w1", 256, "u80", None, 1, 3, 1520, "logits over +-80: expf(80) summed over 256 points"),
    HeadCase("n256_u80_prev1.7", 256, "u80", 1.7, 0, 1, 821, "logits over +-80, composed with a non-unit coarse pose"),
    HeadCase("n256_u100_prev", 256, "u100", 1.0, 0, 2, 1422, "logits over +-100: expf overflows float32 unless the maximum is subtracted"),
    HeadCase("n257_prev_w1025", 257, "randn3", 1.0, 1025, 2, 823, "one point past the unroll; warp's second trip with q_prev"),
    HeadCase("n257_w777", 257, "randn3", None, 777, 0, 124, "one point past the unroll, level-4 form, the old test's warp size"),
    HeadCase("n1000", 1000, "randn3", None, 0, 3, 825, "the old test's shape: 15 trips and a partial one"),
    HeadCase("n1000_prev_w2049", 1000, "randn3", 1.0, 2049, 1, 826, "the product's form at levels 3 and 2: q_prev and a warp of three trips"),
    HeadCase("n1000_w1024", 1000, "randn3", None, 1024, 2, 1027, "the product's level-2 warp size, level-4 form"),
    HeadCase("n1000_prev1.7_w1", 1000, "randn3", 1.7, 1, 0, 228, "non-unit coarse pose feeding the in-launch warp"),
    HeadCase("n1000_prev0.3", 1000, "randn3", 0.3, 0, 2, 229, "non-unit coarse pose, no warp"),
]
HEAD_BY_NAME = {c.name: c for c in HEAD_CASES}

# N, spread, seed of test_masked_pool_against_float64
POOL_CASES = [(1, "randn3", 301), (3, "randn3", 1303), (63, "randn3", 6363), (64, "randn3", 13364), (65, "randn3", 14365),
              (255, "randn3", 6555), (256, "randn3", 1556), (257, "randn3", 13557), (1000, "randn3", 13300),
              (256, "u80", 9556), (65, "u80", 365), (256, "u100", 556)]

HEAD_MUTANTS = ("softmax_without_max", "last_partial_trip_dropped", "composition_swapped", "t_rotated_by_composed_q",
                "row_not_normalised")
MUTANTS = HEAD_MUTANTS + WARP_MUTANTS


@functools.lru_cache(maxsize=None)
def head_weights():
    """[w_qt (256,64,1), b_qt, w_q (4,256,1), b_q, w_t (3,256,1), b_t] filled by ``params.fill_value`` under the
    ``pose_calculator_4`` prefix, as ``test_gpu_fused.filled`` fills the module."""
    shapes = (("conv1d_q_t", (256, 64, 1)), ("conv1d_q", (4, 256, 1)), ("conv1d_t", (3, 256, 1)))
    out = []
    for name, shape in shapes:
        for leaf, s in (("weight", shape), ("bias", shape[:1])):
            out.append(torch.from_numpy(np.array(params.fill_value("%s.%s.conv.%s" % (PREFIX, name, leaf), s))).reshape(s))
    return out


def pool_inputs(N, spread, seed, B=B_HEAD):
    """-> emb, logits (B,N,64) point-major float32."""
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn(B, N, 64, generator=g)
    if spread == "randn3":
        logits = torch.randn(B, N, 64, generator=g) * 3
    else:
        half = {"u80": 80.0, "u100": 100.0}[spread]
        logits = (torch.rand(B, N, 64, generator=g) * 2 - 1) * half
    return emb, logits


def head_inputs(case):
    """-> dict(emb, logits (B,N,64); q_prev (B,4) / t_prev (B,3) or None; warp_next (B,warp_n,3) or None)."""
    emb, logits = pool_inputs(case.N, case.spread, case.seed)
    g = torch.Generator().manual_seed(1000 + case.seed)
    q_prev = t_prev = warp_next = None
    if case.prev is not None:
        q_prev = (F.normalize(torch.randn(B_HEAD, 4, generator=g), dim=1) * case.prev).contiguous()
        t_prev = torch.randn(B_HEAD, 3, generator=g)
    if case.warp_n:
        warp_next = ((torch.rand(B_HEAD, case.warp_n, 3, generator=g) * 2 - 1) * 10).contiguous()
    return dict(emb=emb, logits=logits, q_prev=q_prev, t_prev=t_prev, warp_next=warp_next)


def pool_model(emb, logits, dtype, order="torch", mutant=None):
    """sum_n emb * softmax_n(logits): emb, logits (B,N,64) -> (B,64).  ``order="torch"``: F.softmax and torch.sum on the
    channel-major tensors, as oracle/model.py does.  ``order="slots"``: the kernel's arithmetic -- channel maximum,
    e = exp(logit - max), 64 partial sums of e and of e * emb over points i = slot mod 64 (each in point order), the 64
    partials added one after the other, one division."""
    emb, logits = emb.to(dtype), logits.to(dtype)
    N = emb.shape[1]
    if mutant == "last_partial_trip_dropped" and N % SLOTS:
        emb, logits = emb[:, :N - N % SLOTS], logits[:, :N - N % SLOTS]
        N = emb.shape[1]
    if order == "torch":
        e, m = emb.permute(0, 2, 1).contiguous(), logits.permute(0, 2, 1).contiguous()
        if mutant == "softmax_without_max":
            ex = torch.exp(m)
            w = ex / ex.sum(dim=2, keepdim=True)
        else:
            w = F.softmax(m, dim=2)
        return torch.sum(e * w, dim=2)
    assert order == "slots"
    B = emb.shape[0]
    if N == 0:                                    # the mutant at N < 64: nothing left to sum, 0 / 0
        return torch.zeros(B, 64, dtype=dtype) / torch.zeros(B, 64, dtype=dtype)
    mx = logits.max(dim=1, keepdim=True).values
    ex = torch.exp(logits if mutant == "softmax_without_max" else logits - mx)
    den, num = torch.zeros(B, SLOTS, 64, dtype=dtype), torch.zeros(B, SLOTS, 64, dtype=dtype)
    for i0 in range(0, N, SLOTS):                 # one trip: slot s takes point i0 + s
        k = min(SLOTS, N - i0)
        den[:, :k] = den[:, :k] + ex[:, i0:i0 + k]
        num[:, :k] = num[:, :k] + ex[:, i0:i0 + k] * emb[:, i0:i0 + k]
    d, s = torch.zeros(B, 64, dtype=dtype), torch.zeros(B, 64, dtype=dtype)
    for slot in range(SLOTS):
        d, s = d + den[:, slot], s + num[:, slot]
    return s / d


def _normalise(q, eps):
    """q / (sqrt(|q|^2 + 1e-10) + 1e-10) over the last axis, |q|^2 summed left to right."""
    w, x, y, z = (q[:, i:i + 1] for i in range(4))
    return q / (torch.sqrt((((w * w + x * x) + y * y) + z * z) + eps) + eps)


def normalise_q(q, dtype):
    """The pose row's quaternion (PW/pwclo_net.py:195-198) of q (B,4) in ``dtype``."""
    return _normalise(q.detach().cpu().to(dtype), torch.tensor(1e-10, dtype=dtype))


def head_model(emb, logits, weights, q_prev, t_prev, dtype, order="torch", mutant=None):
    """The eval pose head on the CPU.  emb, logits (B,N,64) point-major; ``weights`` as ``head_weights()``; q_prev (B,4),
    t_prev (B,3) or None.  -> pooled (B,64), q (B,4), t (B,3), pose_row (B,7) = [t, q normalised]."""
    w_qt, b_qt, w_q, b_q, w_t, b_t = (w.to(dtype) for w in weights)
    eps = torch.tensor(1e-10, dtype=dtype)
    pooled = pool_model(emb, logits, dtype, order, mutant)
    big = F.conv1d(pooled.unsqueeze(2), w_qt, b_qt)                       # pose_calculator.py:60
    qd = F.conv1d(big, w_q, b_q).squeeze(2)                               # eval mode: dropout is the identity
    qd = qd / (torch.sqrt(torch.sum(qd * qd, dim=1, keepdim=True) + eps) + eps)
    td = F.conv1d(big, w_t, b_t).squeeze(2)
    if q_prev is None:
        q, t = qd, td
    else:
        qc, tc = q_prev.to(dtype), t_prev.to(dtype)
        cols = lambda v: [v[:, i] for i in range(v.shape[1])]
        left, right = (qc, qd) if mutant == "composition_swapped" else (qd, qc)
        q = torch.stack(_hamilton(cols(left), cols(right)), dim=1)        # mul_point_q(q_det, q_coarse), :139
        rot = q if mutant == "t_rotated_by_composed_q" else qd
        t = torch.stack(_warp_components(cols(rot), cols(tc), cols(td), eps), dim=1)       # warp(t_coarse, q_det, t_det), :148
    row = torch.cat((t, q if mutant == "row_not_normalised" else _normalise(q, eps)), dim=1)
    return pooled, q, t, row


HEAD_OUTPUTS = ("pooled", "q", "t", "row")


@functools.lru_cache(maxsize=None)
def head_reference(name):
    """(float64 outputs, float32 outputs) of ``head_model`` for the case: computed once, shared, never modified."""
    case = HEAD_BY_NAME[name]
    x = head_inputs(case)
    args = (x["emb"], x["logits"], head_weights(), x["q_prev"], x["t_prev"])
    return head_model(*args, torch.float64), head_model(*args, torch.float32)


@functools.lru_cache(maxsize=None)
def pool_reference(N, spread, seed):
    emb, logits = pool_inputs(N, spread, seed)
    return pool_model(emb, logits, torch.float64), pool_model(emb, logits, torch.float32)
