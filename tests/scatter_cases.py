"""The case table of tests/test_gpu_scatter_grads.py, with its inputs and float64 references, shared with
tests/test_scatter_plan_cpu.py, which proves through group_points_grad_plan_query / three_interpolate_grad_plan_query that
the rows reach every form the two dispatches can select and hold both sides of every size threshold.

A scatter-add is ``out[b, c, idx[b, p]] += v[b, c, p]``: for group_points_grad v is the gradient and p runs over the s * k
grouped positions; gather_points_grad is the same with k = 1; three_interpolate_grad scatters the 3 n products
``grad[b, c, j] * weight[b, j, i]``.  Everything here is CPU torch / numpy: the same tensors reach both test files.

A form is (kernel, ct, several position ranges, vec4, channel tail):
  ct      channels per slice: 8 while 8 rows of n floats fit 128 KiB of LDS, then 4 / 2 / 1; min(c, 8) when c < 8; halved
          (3 from 6 or 7) until b * slices reaches 256 workgroups;
  ranges  > 1 only when b * slices < 64 (that implies ct = 1): every range flushes with global atomics;
  vec4    16-byte loads: P % 4 == 0 (torch's allocations and the slices of a concatenated gradient are 16-byte aligned then);
  tail    c % ct != 0: the last slice is narrower.
"""
from collections import namedtuple

import numpy as np
import torch

U = 2.0 ** -24                       # unit roundoff of fp32
RMS_MARGIN = 4.0                     # the project's margin for "another summation order" (stack and conv suites)

# want: ("atomic",) or ("lds", ct, ranges > 1, vec4, tail); opts: "ranges": the number of position ranges the plan must give,
# "short": the last range is shorter than the others, "perm": P == n, the permutation distribution applies
Group = namedtuple("Group", "b c n s k want opts")
Interp = namedtuple("Interp", "b c n m want opts")       # want without the vec4 field
Gather = namedtuple("Gather", "b c n m want opts")       # want: a Group form, or ("gather",) for the n > 32768 kernel


def _g(b, c, n, s, k, want, **opts):
    return Group(b, c, n, s, k, want, opts)


def _i(b, c, n, m, want, **opts):
    return Interp(b, c, n, m, want, opts)


def _ga(b, c, n, m, want, **opts):
    return Gather(b, c, n, m, want, opts)


def _both(b, c, n, s, ct, tail):
    """P = 4 s (vec4) and P = 3 s (scalar loads) of one (b, c, n)."""
    return [_g(b, c, n, s, 4, ("lds", ct, False, 1, tail)), _g(b, c, n, s, 3, ("lds", ct, False, 0, tail))]


GROUP_CASES = (
    # ---- one position range per slice (b * slices >= 256 or ct = 1 with >= 64 slices): plain read-modify-write flush
    _both(32, 64, 64, 37, 8, False) + _both(128, 9, 64, 37, 8, True)
    + _both(256, 7, 64, 9, 7, False) + _both(256, 6, 64, 9, 6, False) + _both(256, 5, 64, 9, 5, False)
    + _both(16, 64, 64, 37, 4, False) + _both(16, 65, 64, 37, 4, True)
    + _both(128, 6, 64, 9, 3, False) + _both(128, 7, 64, 9, 3, True)
    + _both(8, 64, 64, 37, 2, False) + _both(8, 65, 64, 37, 2, True)
    + _both(1, 64, 64, 37, 1, False)
    + [
        # more positions than one pass of the 512 threads takes (2048 with 16-byte loads): a partial last pass
        _g(32, 64, 64, 513, 4, ("lds", 8, False, 1, False)),
        _g(1, 64, 64, 1025, 4, ("lds", 1, False, 1, False)),
        _g(1, 64, 64, 683, 3, ("lds", 1, False, 0, False)),
        # ---- several position ranges (b * slices < 64): equal ranges, P % 4 != 0, a shorter last range, the most ranges
        _g(1, 1, 64, 2048, 4, ("lds", 1, True, 1, False), ranges=4),
        _g(1, 1, 64, 2731, 3, ("lds", 1, True, 0, False), ranges=5, short=True),
        _g(1, 1, 64, 2049, 4, ("lds", 1, True, 1, False), ranges=5, short=True),
        _g(3, 2, 100, 1025, 4, ("lds", 1, True, 1, False), ranges=3, short=True),
        _g(1, 1, 64, 131072, 4, ("lds", 1, True, 1, False), ranges=256),
        # ---- both sides of every size threshold: 8 | 4 | 2 | 1 rows of n floats in 128 KiB, then global atomics
        _g(32, 64, 4096, 37, 4, ("lds", 8, False, 1, False)), _g(32, 64, 4097, 37, 3, ("lds", 4, False, 0, False)),
        _g(16, 64, 8192, 37, 4, ("lds", 4, False, 1, False)), _g(16, 64, 8193, 37, 3, ("lds", 2, False, 0, False)),
        _g(16, 32, 16384, 37, 4, ("lds", 2, False, 1, False)), _g(16, 32, 16385, 37, 3, ("lds", 1, False, 0, False)),
        _g(1, 3, 32768, 1537, 4, ("lds", 1, True, 1, False), ranges=4, short=True),
        _g(1, 3, 32769, 1537, 4, ("atomic",)), _g(2, 9, 32769, 37, 3, ("atomic",)),
        # ---- P == n: every target exactly once
        _g(32, 64, 64, 16, 4, ("lds", 8, False, 1, False), perm=True),
        _g(1, 1, 8192, 2048, 4, ("lds", 1, True, 1, False), ranges=4, perm=True),
        _g(1, 3, 32769, 10923, 3, ("atomic",), perm=True),
    ])

INTERP_CASES = [
    _i(32, 64, 150, 64, ("lds", 8, False, False)), _i(32, 65, 150, 64, ("lds", 8, False, True)),
    _i(256, 7, 50, 64, ("lds", 7, False, False)), _i(256, 6, 50, 64, ("lds", 6, False, False)),
    _i(256, 5, 50, 64, ("lds", 5, False, False)),
    _i(16, 64, 150, 64, ("lds", 4, False, False)), _i(16, 65, 150, 64, ("lds", 4, False, True)),
    _i(128, 6, 50, 64, ("lds", 3, False, False)), _i(128, 7, 50, 64, ("lds", 3, False, True)),
    _i(8, 64, 150, 64, ("lds", 2, False, False)), _i(8, 65, 150, 64, ("lds", 2, False, True)),
    _i(1, 64, 1500, 64, ("lds", 1, False, False)),                    # three passes of the 512 threads, the last partial
    # several ranges of ceil(n / splits) fine points: equal, a shorter last one, the most
    _i(1, 1, 4096, 64, ("lds", 1, True, False), ranges=4),
    _i(1, 1, 4099, 64, ("lds", 1, True, False), ranges=5, short=True),
    _i(3, 2, 2049, 100, ("lds", 1, True, False), ranges=3),
    _i(1, 1, 261121, 64, ("lds", 1, True, False), ranges=256),
    _i(32, 64, 150, 4096, ("lds", 8, False, False)), _i(32, 64, 150, 4097, ("lds", 4, False, False)),
    _i(16, 64, 150, 8192, ("lds", 4, False, False)), _i(16, 64, 150, 8193, ("lds", 2, False, False)),
    _i(16, 32, 150, 16384, ("lds", 2, False, False)), _i(16, 32, 150, 16385, ("lds", 1, False, False)),
    _i(1, 3, 3000, 32768, ("lds", 1, True, False), ranges=3),
    _i(1, 3, 3000, 32769, ("atomic",)), _i(2, 9, 300, 32769, ("atomic",)),
    # 3 n == m: every target exactly once
    _i(32, 64, 50, 150, ("lds", 8, False, False), perm=True),
    _i(1, 1, 4096, 12288, ("lds", 1, True, False), ranges=4, perm=True),
    _i(1, 3, 10923, 32769, ("atomic",), perm=True),
]

# gather_points_grad: group_points_grad with k = 1 up to n = 32768, its own kernel (one thread per (channel, position), grid
# y = c) beyond; m = 1 and the odd channel count c = 65 in both
GATHER_CASES = [
    _ga(32, 64, 64, 148, ("lds", 8, False, 1, False)), _ga(2, 65, 64, 1, ("lds", 1, False, 0, False)),
    _ga(2, 65, 300, 299, ("lds", 1, False, 0, False)), _ga(1, 1, 64, 8193, ("lds", 1, True, 0, False)),
    _ga(1, 3, 32768, 6148, ("lds", 1, True, 1, False)),
    _ga(1, 3, 32769, 6148, ("gather",)), _ga(2, 65, 32769, 1, ("gather",)), _ga(2, 65, 40000, 515, ("gather",)),
    # m == n: every target exactly once, through the LDS kernel (one range, several) and through the kernel of its own
    _ga(2, 65, 300, 300, ("lds", 1, False, 1, False), perm=True),
    _ga(1, 3, 8192, 8192, ("lds", 1, True, 1, False), perm=True),
    _ga(1, 3, 32769, 32769, ("gather",), perm=True),
]

THRESHOLDS = (4096, 8192, 16384, 32768)       # the last n (or m) of 8, 4, 2, 1 rows in LDS; 32769: global atomics
DISTRIBUTIONS = ("uniform", "first", "last", "edges", "clustered")        # + "permutation" where the case has P == n


def case_id(c):
    return "-".join(str(v) for v in c if isinstance(v, int)) + "-" + "_".join(str(int(v)) if not isinstance(v, str) else v
                                                                             for v in c.want)


def kinds(case):
    """Value kinds of a case: see ``make_values``."""
    return ("int", "int01", "real") if isinstance(case, Interp) else ("int", "real")


def group_form(plan, c):
    """The form of a *_grad_plan_query answer (``_ext.group_points_grad_plan`` dict) for c channels."""
    if plan["form"] == "atomic":
        return ("atomic",)
    return ("lds", plan["ct"], plan["ranges"] > 1, plan["vec4"], c % plan["ct"] != 0)


def interp_form(plan, c):
    f = group_form(plan, c)
    return f if f == ("atomic",) else f[:3] + f[4:]


def positions(case):
    """Number of scattered values per (cloud, channel) and of targets."""
    if isinstance(case, Group):
        return case.s * case.k, case.n
    if isinstance(case, Interp):
        return 3 * case.n, case.m
    return case.m, case.n


def distributions(case):
    P, n = positions(case)
    perm = case.opts.get("perm", False)
    assert not perm or P == n
    return DISTRIBUTIONS + (("permutation",) if perm else ())


def _seed(case, dist, salt=0):
    P, n = positions(case)
    return (case.b * 1000003 + case.c * 7919 + P * 31 + n + 97 * (DISTRIBUTIONS + ("permutation",)).index(dist) + salt) % (2 ** 31)


def make_idx(case, dist):
    """(b, P) int32 targets in [0, n) (callers view it as (b, s, k) / (b, n, 3) / (b, m))."""
    P, n = positions(case)
    b = case.b
    gen = torch.Generator().manual_seed(_seed(case, dist))
    if dist == "uniform":
        return torch.randint(0, n, (b, P), generator=gen, dtype=torch.int32)
    if dist == "first":
        return torch.zeros((b, P), dtype=torch.int32)
    if dist == "last":
        return torch.full((b, P), n - 1, dtype=torch.int32)
    if dist == "edges":
        return torch.tensor([0, 1, n - 2, n - 1], dtype=torch.int32)[torch.randint(0, 4, (b, P), generator=gen)]
    if dist == "permutation":
        return torch.stack([torch.randperm(n, generator=gen) for _ in range(b)]).to(torch.int32)
    # clustered: the neighbour lists of queries in three tight clusters inside a spread-out cloud of n points -- a few hot
    # targets, the rest untouched.  A few clouds are searched; the batch repeats them.
    from oracle import ops as O
    kk = 1 if isinstance(case, Gather) else (3 if isinstance(case, Interp) else case.k)
    kk = min(kk, n)
    S = -(-P // kk)
    nb = min(b, 3)
    cloud = (torch.rand(nb, n, 3, generator=gen) * 2 - 1) * 10
    centres = cloud[:, torch.randint(0, n, (3,), generator=gen)]                                   # (nb, 3, 3)
    q = centres[:, torch.randint(0, 3, (S,), generator=gen)] + torch.randn(nb, S, 3, generator=gen) * 0.05
    _, idx = O.knn_point_with_dist(kk, cloud.contiguous(), q.contiguous())
    idx = idx.reshape(nb, -1)[:, :P]
    return idx[torch.arange(b) % nb].contiguous()


def make_values(case, kind, dist):
    """-> (v (b, c, P) fp32 as the kernel adds them, v64 the same products in float64 (exact), parts).  ``parts``: what
    the op takes -- (grad,) for group / gather, (grad (b, c, n), weight (b, n, 3)) for interpolate.  kind "int": integers in
    [-8, 8], weights from {0.25, 0.5, 1, 2}; "int01" (interpolate): weights from {0, 1}, so exact zeros are added; "real":
    randn, weights rand."""
    P, n = positions(case)
    b, c = case.b, case.c
    gen = torch.Generator().manual_seed(_seed(case, dist, 1 + ("int", "int01", "real").index(kind)))
    npos = case.n if isinstance(case, Interp) else P
    if kind != "real":
        g = torch.randint(-8, 9, (b, c, npos), generator=gen).float()
    else:
        g = torch.randn(b, c, npos, generator=gen)
    if not isinstance(case, Interp):
        return g, g.double(), (g,)
    if kind != "real":
        table = torch.tensor([0.0, 1.0]) if kind == "int01" else torch.tensor([0.25, 0.5, 1.0, 2.0])
        w = table[torch.randint(0, len(table), (b, npos, 3), generator=gen)]
    else:
        w = torch.rand(b, npos, 3, generator=gen)
    v = (g.unsqueeze(3) * w.unsqueeze(1)).reshape(b, c, P)                       # one fp32 rounding per product
    v64 = (g.double().unsqueeze(3) * w.double().unsqueeze(1)).reshape(b, c, P)   # 24 x 24 bits: exact in float64
    return v, v64, (g, w)


def exact(v64, idx, n):
    """float64 sums -> (out (b, c, n), count (b, n), sum of |contribution| (b, c, n))."""
    b, c, P = v64.shape
    ix = idx.long().unsqueeze(1).expand(b, c, P)
    out = torch.zeros((b, c, n), dtype=torch.float64).scatter_add_(2, ix, v64)
    mag = torch.zeros((b, c, n), dtype=torch.float64).scatter_add_(2, ix, v64.abs())
    cnt = torch.zeros((b, n), dtype=torch.float64).scatter_add_(1, idx.long(), torch.ones((b, P), dtype=torch.float64))
    return out, cnt, mag


def index_add32(v, idx, n, reverse=False):
    """torch's fp32 ``index_add_`` on the CPU, positions forward or reversed."""
    b, c, P = v.shape
    out = torch.zeros((b, c, n), dtype=torch.float32)
    for i in range(b):
        ix, vi = idx[i].long(), v[i]
        if reverse:
            ix, vi = ix.flip(0), vi.flip(1)
        out[i].index_add_(1, ix, vi.contiguous())
    return out


def sequential32(v, idx, n):
    """Every target's contributions added one by one in ascending position with fp32 rounding at each step, from 0: the
    order group_points_grad_sorted_kernel states (numpy's unbuffered ``add.at`` walks the positions in order)."""
    b, c, P = v.shape
    out = np.zeros((b, c, n), dtype=np.float32)
    vn, ixn = v.numpy(), idx.numpy().astype(np.intp)
    for i in range(b):
        for ch in range(c):
            np.add.at(out[i, ch], ixn[i], vn[i, ch])
    return torch.from_numpy(out)


def gamma(k):
    """gamma_k = k u / (1 - k u): |fl(sum of k fp32 terms, any order) - sum| <= gamma_(k-1) sum |terms|."""
    return k * U / (1 - k * U)


def rounding_bound(cnt, mag):
    """Per target: gamma_(count + 1) * sum |contribution|  (b, c, n); the + 1 covers the product in interpolate and the final
    add into the zero-filled buffer."""
    return (gamma(cnt + 1)).unsqueeze(1) * mag


def rms(t):
    return float(t.double().pow(2).mean().sqrt())
