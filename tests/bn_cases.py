"""The case tables of tests/test_gpu_bn_variants.py, with their inputs, float64 references and error bounds, shared with
tests/test_bn_plan_cpu.py, which proves through batchnorm_train_plan_query (``batchnorm.plan``) that the rows reach every
form the launchers of csrc/batchnorm.hip can select, that the exact cases are exact in fp32 and that the bounds hold for
an fp32 evaluation of the kernels' expressions.  Everything here is CPU torch / numpy.

A dense form is (vec, split class, row class, c % 4) of a (b, c, L) problem, M = b * L positions per channel:
  vec     L % 4 == 0: 16-byte loads in bn_partial_kernel and bn_apply_kernel<., true, .>, else the scalar paths;
  split   nsplit of the reduction passes: "1" | "2..64" | "65..255" (bn_fold's lanes take several partials) | "256" (the cap);
  row     "short": L below one step of the 256 threads (1024 elements vec, 256 scalar), the (b, l) walk crosses several rows
          per step; "long": L > per_split, a range begins and ends inside a row; "mid" otherwise;
  c % 4   the finish kernels take 4 channels per workgroup.
Kernels per case: bn_partial_kernel<0, false>, bn_forward_finish_kernel, bn_apply_kernel<0, vec, relu> (forward),
bn_partial_kernel<1, relu>, bn_backward_finish_kernel, bn_apply_kernel<1, vec, relu> (backward): a case with vec = 0 and the
configuration relu = 1 is what reaches bn_apply_kernel<0, false, true> / <1, false, true>, and so on.

A max-K form is (K, vec of the backward reduction = S % 4 == 0, several splits in that reduction, partial last wave =
(S * K / 4) % 256 != 0): bn_apply_relu_maxk_kernel<K>, bn_apply_bwd_maxk_kernel<K>, bn_partial_kernel<1, true> on (c, b * S, S).
The split classes beyond 64 of that reduction would need b * S > 262144 rows (x of at least 4 MB ... 67 MB); bn_fold with
more than 64 partials is the dense cases' business, so the max-K table only tells one split from several.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

U = 2.0 ** -24                       # unit roundoff of fp32
U64 = 2.0 ** -53                     # ... of fp64
TINY = 2.0 ** -126                   # smallest normal fp32: results below it may be flushed to 0
EPS = float(np.float32(1e-5))        # the entry points take eps as a float: the references use that value
MOMENTUM = 0.1

Dense = namedtuple("Dense", "b c L want opts")     # want: the form; opts: "short_last": the last split is shorter
MaxK = namedtuple("MaxK", "b c S K want")

# (relu, affine, running statistics given): every value of each switch, affine = 0 with relu = 1 among them
CONFIGS = ((0, 1, 1), (1, 1, 0), (1, 0, 1), (0, 0, 0))
FAMILIES = ("gauss", "offset", "const")
SOFTMAX_K = (1, 2, 4, 6, 8, 16, 32)
SOFTMAX_ROWS = (1, 255, 256, 257)


def gamma(k):
    """gamma_k = k u / (1 - k u): a product of k factors (1 + d), |d| <= u, is within gamma_k of 1."""
    return k * U / (1 - k * U)


def gamma64(k):
    return k * U64 / (1 - k * U64)


def split_class(nsplit):
    return "1" if nsplit == 1 else ("2..64" if nsplit <= 64 else ("65..255" if nsplit < 256 else "256"))


def row_class(L, vec, per_split):
    return "short" if L < (1024 if vec else 256) else ("long" if L > per_split else "mid")


def dense_form(plan, c, L):
    return (plan["vec"], split_class(plan["nsplit"]), row_class(L, plan["vec"], plan["per_split"]), c % 4)


def maxk_form(plan, S, K):
    """plan: of the backward reduction, (c, b * S, S)."""
    return (K, plan["vec"], plan["nsplit"] > 1, (S * K // 4) % 256 != 0)


# (b, L) per (vec, split class, row class); every shape with c in 1..4 (2048 / c >= 256 splits wanted: the plan does not
# depend on c there), so that each form meets each residue of c.  The "256" rows are 4 MB per channel: c in {1, 2} only --
# residues 3 and 0 would take 12 and 16 MB tensors (EXEMPT below).
_SHAPES = (
    # ---- one split (M <= 4096): several loop iterations on both paths, rows shorter than a step
    (1, "1", "short", 1000, 4), (1, "1", "mid", 2, 2044),
    (0, "1", "short", 4001, 1), (0, "1", "short", 803, 5), (0, "1", "mid", 3, 1365),
    # ---- several splits of 4096: a boundary inside a row, a shorter last split
    (1, "2..64", "short", 2500, 4), (1, "2..64", "mid", 9, 1028), (1, "2..64", "long", 2, 10004),
    (0, "2..64", "short", 5000, 1), (0, "2..64", "short", 2001, 5), (0, "2..64", "mid", 9, 1027),
    (0, "2..64", "long", 2, 10003),
    # ---- more than 64 splits: bn_fold's s += 64 loop in both finish kernels
    (1, "65..255", "short", 22000, 12), (1, "65..255", "mid", 130, 2052), (1, "65..255", "long", 2, 133336),
    (0, "65..255", "short", 20300, 13), (0, "65..255", "mid", 130, 2051), (0, "65..255", "long", 2, 133335),
    # ---- the cap of 256 splits (M > 255 * 4096)
    (1, "256", "short", 65300, 16), (1, "256", "mid", 511, 2052), (1, "256", "long", 2, 524292),
    (0, "256", "short", 61500, 17), (0, "256", "mid", 512, 2051), (0, "256", "long", 2, 524291),
)

DENSE_CASES = [Dense(b, c, L, (vec, sc, rc, c % 4), {"short_last": True})
               for (vec, sc, rc, b, L) in _SHAPES for c in ((1, 2) if sc == "256" else (1, 2, 3, 4))]
DENSE_CASES += [
    # a full finish workgroup followed by a partial one, several splits; fewer splits wanted than 256 (2048 / 33 = 62)
    Dense(9, 5, 1028, (1, "2..64", "mid", 1), {"short_last": True}), Dense(9, 6, 1027, (0, "2..64", "mid", 2), {"short_last": True}),
    Dense(9, 7, 1028, (1, "2..64", "mid", 3), {"short_last": True}), Dense(2, 33, 10003, (0, "2..64", "long", 1), {"short_last": True}),
    Dense(2, 8, 8192, (1, "2..64", "long", 0), {}),                  # equal splits, the last one full
]

# forms the unrestricted sweep finds and the table leaves out, with the reason: c * M * 4 bytes > 8 MB
EXEMPT = {(vec, "256", rc, r) for vec in (0, 1) for rc in ("short", "mid", "long") for r in (3, 0)}

MAXK_CASES = []
for _K in (4, 8, 16, 32):
    # S: a multiple of 4 with full waves, with a partial last wave; S % 4 != 0; one row; b * S > 4096 (several splits in the
    # backward reduction) with S % 4 == 0 partial, full, and S % 4 != 0
    for _b, _c, _S in ((2, 3, 256), (3, 5, 36), (3, 2, 37), (2, 4, 1), (2, 3, 2052), (2, 1, 2304), (2, 3, 2051)):
        MAXK_CASES.append(MaxK(_b, _c, _S, _K, (_K, int(_S % 4 == 0), _b * _S > 4096, (_S * _K // 4) % 256 != 0)))


def dense_id(case):
    return "b%d-c%d-L%d-%s-s%s-%s" % (case.b, case.c, case.L, "vec" if case.want[0] else "scalar", case.want[1], case.want[2])


def maxk_id(case):
    return "b%d-c%d-S%d-K%d" % (case.b, case.c, case.S, case.K)


def _seed(*v):
    s = 12345
    for t in v:
        s = (s * 1000003 + int(t)) % (2 ** 31 - 1)
    return s


# ---- real-valued inputs ---------------------------------------------------------------------------------------------

def dense_input(case, family):
    """x (b, c, L) fp32.  gauss: N(0.3, 1.7); offset: mean 6144, std 1.5 (mean / std = 2^12; mean^2 lies inside a binade,
    where fp32 squares are 4 apart: with mean 4096 = 2^12 exactly they straddle 2^24 and an fp32 variance can land on
    1 by luck); const: channel 0 constant."""
    gen = torch.Generator().manual_seed(_seed(case.b, case.c, case.L, FAMILIES.index(family)))
    x = torch.randn(case.b, case.c, case.L, generator=gen)
    if family == "offset":
        return x * 1.5 + 6144.0
    x = x * 1.7 + 0.3
    if family == "const":
        x[:, 0] = 3.25
    return x


def dense_grad(case):
    gen = torch.Generator().manual_seed(_seed(case.b, case.c, case.L, 77))
    return torch.randn(case.b, case.c, case.L, generator=gen)


def affine_params(c, affine, signed=True):
    """gamma, beta (c) fp32 or (None, None).  gamma alternates in sign (negative gamma: the max over K comes from the smallest
    x), magnitudes in [0.5, 1.5]."""
    if not affine:
        return None, None
    g = torch.linspace(0.5, 1.5, c) if c > 1 else torch.tensor([0.75])
    if signed:
        g = g * torch.tensor([1.0, -1.0]).repeat(c)[:c]
    be = torch.linspace(-0.3, 0.4, c) if c > 1 else torch.tensor([0.2])
    return g.float().contiguous(), be.float().contiguous()


def running_init(c):
    return torch.linspace(-0.5, 0.5, c).float() if c > 1 else torch.tensor([0.25]), \
        torch.linspace(0.5, 1.5, c).float() if c > 1 else torch.tensor([0.8])


def maxk_input(case):
    """x (b, c, S, K): Gaussian, and in a random half of the rows x[..., 0] copied into a random subset of the other
    positions (grouped neighbourhoods are padded with repeated neighbours: exact ties inside a row)."""
    gen = torch.Generator().manual_seed(_seed(case.b, case.c, case.S, case.K, 5))
    x = torch.randn(case.b, case.c, case.S, case.K, generator=gen) * 1.7 + 0.3
    dup = (torch.rand(case.b, case.c, case.S, case.K, generator=gen) < 0.4) & \
          (torch.rand(case.b, case.c, case.S, 1, generator=gen) < 0.5)
    x = torch.where(dup, x[..., :1].expand_as(x), x).contiguous()
    dpool = torch.randn(case.b, case.c, case.S, generator=gen)
    return x, dpool


# ---- float64 references and bounds ----------------------------------------------------------------------------------

def stats_reference(x, eps=EPS):
    """Two-pass float64 statistics of the fp32 data -> dict of (c) float64 tensors and the magnitudes of the bounds."""
    x64 = x.double().transpose(0, 1).reshape(x.shape[1], -1)
    M = x64.shape[1]
    mean = x64.mean(1)
    var = (x64 - mean[:, None]).pow(2).mean(1)
    return dict(M=M, mean=mean, var=var, invstd=1.0 / torch.sqrt(var + eps), unbiased=var * M / max(M - 1, 1),
                mean_abs=x64.abs().mean(1), mean_sq=x64.pow(2).mean(1))


def stats_bounds(ref, eps=EPS):
    """|mean - ref| <= U |ref| + gamma64(M) mean|x| (one rounding to fp32 of a fp64 sum of M terms);
    |var - ref| <= 2 gamma64(M) mean(x^2) (the sums of x^2 and, squared, of x), propagated to invstd = (var + eps)^-1/2 as
    U invstd + 1/2 invstd var_err / (var + eps)."""
    M = ref["M"]
    bm = U * ref["mean"].abs() + gamma64(M) * ref["mean_abs"]
    bv = 2 * gamma64(M) * ref["mean_sq"]
    bi = U * ref["invstd"] + 0.5 * ref["invstd"] * bv / (ref["var"] + eps)
    return bm, bv, bi


def running_reference(ref, rm0, rv0, momentum=MOMENTUM):
    """The kernel's update in float64 with the fp32 momentum; bounds: the statistic's own, scaled, and one more U relative."""
    m = float(np.float32(momentum))
    bm, bv, _ = stats_bounds(ref)
    M = ref["M"]
    rm = (1.0 - m) * rm0.double() + m * ref["mean"]
    rv = (1.0 - m) * rv0.double() + m * ref["unbiased"]
    return rm, rv, m * bm + U * rm.abs(), m * bv * M / max(M - 1, 1) + U * rv.abs()


def _bc(t, like):
    """(c) -> broadcast against (b, c, ...)."""
    return t.reshape((1, -1) + (1,) * (like.dim() - 2))


N_Y = 4       # y = ((x - mu) * is) * g + be: subtraction, two products, sum (3 when the last two contract into an FMA)
N_DX = 6      # dx = ((gv - c0) - xh * c1) * (g * is) with c0, c1 as the kernel rounds them: the xh * c1 term passes the two
              # roundings of xh, its product, one subtraction, the final product and the rounding of g * is; gv and c0 pass 4


def forward_reference(x, mean, invstd, g, be):
    """float64 y before the ReLU from the kernel's own fp32 mean / invstd, and its per-element bound
    gamma(N_Y) (|xhat g| + |be|)."""
    x64 = x.double()
    xh = (x64 - _bc(mean.double(), x64)) * _bc(invstd.double(), x64)
    g64 = _bc(g.double(), x64) if g is not None else 1.0
    b64 = _bc(be.double(), x64) if be is not None else 0.0
    y = xh * g64 + b64
    bound = gamma(N_Y) * ((xh * g64).abs() + (b64.abs() if be is not None else 0.0))
    return y, bound, xh


def kernel_c01(dgamma, dbeta, M):
    """c0 = dbeta * inv_m, c1 = dgamma * inv_m exactly as the kernels round them: inv_m = (float)(1.0 / M), one fp32 product."""
    inv_m = np.float32(1.0 / float(M))
    return torch.from_numpy(dbeta.numpy() * inv_m), torch.from_numpy(dgamma.numpy() * inv_m)


def backward_reference(xh, gv, invstd, g, c0, c1):
    """float64 dx for the (masked) gradient gv from the kernel's own c0 / c1, and the bound gamma(N_DX) |g is| (|gv| + |c0| +
    |xhat c1|)."""
    gi = (_bc(g.double(), xh) if g is not None else 1.0) * _bc(invstd.double(), xh)
    c0b, c1b = _bc(c0.double(), xh), _bc(c1.double(), xh)
    dx = ((gv - c0b) - xh * c1b) * gi
    bound = gamma(N_DX) * abs(gi) * (gv.abs() + c0b.abs() + (xh * c1b).abs())
    return dx, bound


def sums_reference(xh, gv, slack=None):
    """dbeta = sum gv, dgamma = sum gv xhat over (b, positions) in float64, with |dbeta - ref| <= U |ref| + gamma64(M) sum|gv|,
    dgamma the same + 3 U sum|gv xhat| (the fp32 xhat the kernel multiplies with carries two roundings, the masked product is
    rounded to fp64 once more).  ``slack``: |dy| at the elements whose ReLU decision is within rounding of zero and 0 elsewhere
    (either decision is a correct fp32 evaluation there): added to the bounds."""
    c = xh.shape[1]
    red = lambda t: t.transpose(0, 1).reshape(c, -1).sum(1)
    M = xh.numel() // c
    dbeta, dgamma = red(gv), red(gv * xh)
    sa, sax = red(gv.abs()), red((gv * xh).abs())
    bb = U * dbeta.abs() + gamma64(M) * sa
    bg = U * dgamma.abs() + gamma64(M) * sax + 3 * U * sax
    if slack is not None:
        bb = bb + red(slack)
        bg = bg + red(slack * xh.abs())
    return dgamma, dbeta, bg, bb


# ---- fp32 emulation of the kernels' expressions (numpy; fma: a * b + c rounded once from float64) ---------------------

def _f32(a):
    return np.asarray(a, dtype=np.float32)


def fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate_y(x, mu, is_, g, be, fma):
    """bn_apply_kernel / bn_apply_relu_maxk_kernel: yv = ((x - mu) * is) * g + be in fp32 -> (yv, xh)."""
    x, mu, is_, g, be = _f32(x), _f32(mu), _f32(is_), _f32(g), _f32(be)
    xh = (x - mu) * is_
    return (fma32(xh, g, be) if fma else xh * g + be), xh


def emulate_dx(xh, gv, c0, c1, g, is_, fma):
    """((gv - c0) - xh * c1) * (g * is) in fp32."""
    xh, gv, c0, c1, g, is_ = _f32(xh), _f32(gv), _f32(c0), _f32(c1), _f32(g), _f32(is_)
    t = gv - c0
    t = fma32(-xh, c1, t) if fma else t - xh * c1
    return t * (g * is_)


# ---- exact boundary and tie cases -----------------------------------------------------------------------------------

# per channel (gamma, beta): every gamma of {1, -1, 0.5, 2, 0}, beta a multiple of 1/8 (1/4 where gamma = 2, so that
# y = 0 is reached by a multiple of 1/8); gamma = 0 with beta > 0, = 0 and < 0
EXACT_GB = ((1.0, 0.0), (1.0, -0.375), (-1.0, 0.125), (0.5, -0.25), (2.0, 0.5), (0.0, 0.25), (0.0, 0.0), (0.0, -0.125))
KIND_RANDOM, KIND_ZERO, KIND_PLUS, KIND_MINUS, KIND_NONPOS, KIND_UNIQUE, KIND_TIE = range(7)


@functools.lru_cache(maxsize=None)
def exact_maxk(K, b, S):
    """-> x (b, C, S, K) multiples of 1/8 in [-4, 4], gamma, beta (C), kind (S) and (S, 2) int: the row's construction.
    Rows, the same in every cloud and channel up to the channel's affine map (t = x sorted by y = gamma x + beta):
      ZERO / PLUS / MINUS  the row's largest y is exactly 0 / the smallest positive multiple |gamma| / 8 / its negative
      NONPOS               every y <= 0, random
      UNIQUE (p, -)        the one largest y sits at position p, positive
      TIE (i, j)           the largest y at positions i < j and nowhere else
      RANDOM               random multiples (ties of the maximum are frequent)
    gamma = 0 channels: the whole row ties whatever x is."""
    gen = torch.Generator().manual_seed(_seed(K, b, S, 9))
    C = len(EXACT_GB)
    kinds, where = [], []
    for kd in (KIND_ZERO, KIND_PLUS, KIND_MINUS, KIND_NONPOS):
        kinds += [kd, kd]
        where += [(0, 0), (0, 0)]
    for p in range(K):
        kinds.append(KIND_UNIQUE)
        where.append((p, p))
    for i in range(K):
        for j in range(i + 1, K):
            kinds.append(KIND_TIE)
            where.append((i, j))
    kinds, where = kinds[:S], where[:S]
    kinds += [KIND_RANDOM] * (S - len(kinds))
    where += [(0, 0)] * (S - len(where))
    x = torch.zeros(b, C, S, K)
    for ch, (g, be) in enumerate(EXACT_GB):
        sg = -1.0 if g < 0 else 1.0
        x0 = 0.0 if g == 0 else -be / g                     # y(x0) = 0; a multiple of 1/8 by the choice of EXACT_GB
        for s in range(S):
            kd, (i, j) = kinds[s], where[s]
            # u: multiples of 1/8 in the direction of growing y, relative to the row's top value
            below = -torch.randint(1, 9, (b, K), generator=gen).float() / 8.0          # strictly below the top
            if kd == KIND_RANDOM:
                row = torch.randint(-32, 33, (b, K), generator=gen).float() / 8.0
            elif kd in (KIND_ZERO, KIND_PLUS, KIND_MINUS, KIND_NONPOS):
                top = x0 + sg * {KIND_ZERO: 0.0, KIND_PLUS: 0.125, KIND_MINUS: -0.125, KIND_NONPOS: -0.5}[kd]
                row = top + sg * below
                pos = torch.randint(0, K, (b,), generator=gen)
                row[torch.arange(b), pos] = top
                if kd != KIND_NONPOS:                                                # a second copy of the top: a tie at it
                    row[torch.arange(b), torch.randint(0, K, (b,), generator=gen)] = top
            else:
                top = x0 + sg * 1.5                                                  # y = 1.5 |gamma| > 0
                row = top + sg * below
                row[:, i] = top
                row[:, j] = top
            x[:, ch, s] = row
    assert float(x.abs().max()) <= 4.0 and torch.equal(x * 8, (x * 8).round())
    gb = torch.tensor(EXACT_GB)
    return x.contiguous(), gb[:, 0].contiguous(), gb[:, 1].contiguous(), np.array(kinds), np.array(where)


def exact_dpool(b, C, S, K):
    gen = torch.Generator().manual_seed(_seed(b, C, S, K, 3))
    return torch.randint(-8, 9, (b, C, S), generator=gen).float()


def maxk_reference(x, y):
    """y (b, c, S, K) float64, before the ReLU -> pooled (float64), arg (uint8: the first k reaching it), xsel."""
    r = y.clamp_min(0.0)
    pooled = r.max(dim=3)[0]
    arg = (r == pooled.unsqueeze(3)).to(torch.uint8).argmax(dim=3)      # argmax of 0 / 1: the first 1
    xsel = x.gather(3, arg.unsqueeze(3)).squeeze(3)
    return pooled, arg.to(torch.uint8), xsel


def scatter_dpool(dpool, arg, pooled, K):
    """The dense gradient the max-K backward never writes: dpool at (row, arg) where pooled > 0."""
    dy = torch.zeros(dpool.shape + (K,), dtype=dpool.dtype)
    dy.scatter_(3, arg.long().unsqueeze(3), (dpool * (pooled > 0).to(dpool.dtype)).unsqueeze(3))
    return dy


# ---- softmax weighted sum -------------------------------------------------------------------------------------------

SOFTMAX_KINDS = ("gauss", "equal", "underflow")


def softmax_input(K, rows, kind):
    """x, v (1, 1, rows, K), dout (1, 1, rows).  equal: one logit per row, integer v and dout; underflow: part of each row
    more than 104 below its maximum (expf gives 0 there; down to -88 it is subnormal or flushed)."""
    gen = torch.Generator().manual_seed(_seed(K, rows, SOFTMAX_KINDS.index(kind)))
    x = torch.randn(1, 1, rows, K, generator=gen) * 3
    v = torch.randn(1, 1, rows, K, generator=gen)
    go = torch.randn(1, 1, rows, generator=gen)
    if kind == "equal":
        x = (torch.randn(1, 1, rows, 1, generator=gen) * 3).expand(1, 1, rows, K).contiguous()
        v = torch.randint(-8, 9, (1, 1, rows, K), generator=gen).float()
        go = torch.randint(-8, 9, (1, 1, rows), generator=gen).float()
    elif kind == "underflow":
        drop = torch.tensor([0.0, -50.0, -87.0, -95.0, -110.0, -300.0])[torch.randint(0, 6, (1, 1, rows, K), generator=gen)]
        x = x + drop
    return x.contiguous(), v.contiguous(), go.contiguous()


def softmax_reference(x, v, go):
    """float64 out / dx / dv and row-wise bounds.  With D = max|x - m|: exp's argument carries U |x - m| (relative error of
    the exponential), a 1-ulp expf 2 U, the sum of K terms (K - 1) U, the division U: p_k within (K + 2 + D) U, each product
    and the K-term sum of out (K + 1) U more -- the stated (K + 4 + D) U sum p_k |v_k| holds the first-order terms with K to
    spare; a p_k below the smallest normal may be flushed: TINY per term."""
    x64, v64, g64 = x.double(), v.double(), go.double()
    K = x.shape[3]
    m = x64.max(dim=3, keepdim=True)[0]
    D = (x64 - m).abs().max(dim=3)[0]
    p = torch.softmax(x64, dim=3)
    out = (p * v64).sum(3)
    r = (K + 4 + D) * U
    b_out = r * (p * v64.abs()).sum(3) + TINY * v64.abs().sum(3)
    dv = g64.unsqueeze(3) * p
    b_dv = r.unsqueeze(3) * dv.abs() + TINY * g64.abs().unsqueeze(3)
    diff = v64 - out.unsqueeze(3)
    dx = dv * diff
    # gv_k (its own bound) times (v_k - out): the difference carries out's error and one rounding, the product one more
    b_dx = dv.abs() * (((K + 6 + D) * U).unsqueeze(3) * diff.abs() + b_out.unsqueeze(3)) + TINY * (g64.abs().unsqueeze(3) * diff.abs())
    return (out, dx, dv), (b_out, b_dx, b_dv)


def emulate_softmax(x, v, go):
    """softmax_wsum.hip's row expression in numpy fp32 (np.exp in fp32 for expf; sequential sums)."""
    x, v, go = x.numpy()[0, 0], v.numpy()[0, 0], go.numpy()[0, 0]
    K = x.shape[1]
    m = x.max(axis=1, keepdims=True)
    e = np.exp((x - m).astype(np.float32)).astype(np.float32)
    den = np.zeros(x.shape[0], dtype=np.float32)
    for i in range(K):
        den = den + e[:, i]
    p = e / den[:, None]
    out = np.zeros(x.shape[0], dtype=np.float32)
    for i in range(K):
        out = out + p[:, i] * v[:, i]
    gv = go[:, None] * p
    gx = gv * (v - out[:, None])
    return out, gx, gv
