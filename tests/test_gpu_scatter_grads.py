"""The kernels that carry gradients back through grouping, gathering and interpolation (csrc/group_points.hip,
csrc/interpolate.hip, csrc/sampling.hip: scatter-adds), form by form, against float64 (run with ``-m gpu``).

Every case of tests/scatter_cases.py first asserts through the plan query that its shape selects the form it is meant for
(tests/test_scatter_plan_cpu.py proves the table reaches every reachable one), then runs the op through the ``_ext`` entry
the modules use, for five or six index distributions -- uniform, one target (first / last row of a slice), the four edge
targets, a few hot targets (neighbour lists of clustered queries), a permutation where P == n -- and two kinds of values:

integer-valued   every partial sum in every order is exact in fp32 (shown on the CPU for the reference in two orders), so
                 the atomic, LDS and sorted forms alike must be ``torch.equal`` to the float64 sums; untouched targets
                 are +0.0.  A dropped, doubled or misrouted contribution anywhere fails.
real-valued      per target |got - exact| <= gamma_k * sum |contribution|, k = count + 1, gamma_k = k u / (1 - k u),
                 u = 2^-24: the bound of a k-term fp32 sum in any order (the + 1: the product in interpolate, the final add
                 into the zero-filled buffer).  Derived, no margin.  It is loose at large counts, so the RMS error is also
                 held to 4x that of torch's fp32 index_add_ on the CPU for the uniform and clustered distributions (the
                 suite's margin for another summation order), and ``pytest -s`` prints worst and RMS ratios
                 (profiles/scatter_grads/README.md records them).  The sorted form is bit-identical from run to run and
                 equals the sequential fp32 sum in ascending position.
"""
import contextlib

import pytest
import torch

import scatter_cases as T
from pwclonet_pylidarslam_amd.pointnet2_ops import _ext as E
from pwclonet_pylidarslam_amd.pointnet2_ops import pointnet2_utils as PU

pytestmark = pytest.mark.gpu


class Ref:
    """float64 reference of one (case, distribution, kind) on the device, and what the criteria need."""

    def __init__(self, v, v64, idx, n, dev, kind, dist, need_sequential):
        want, cnt, mag = T.exact(v64, idx, n)
        self.kind, self.dist = kind, dist
        self.exact_eq = kind != "real" or dist == "permutation"
        self.want32 = want.float().to(dev)
        self.untouched = (cnt == 0).unsqueeze(1).expand_as(want).to(dev)
        self.any_untouched = bool((cnt == 0).any())
        if not self.exact_eq:
            self.want = want.to(dev)
            self.bound = T.rounding_bound(cnt, mag).to(dev)
            cpu = (T.index_add32(v, idx, n).double() - want).abs()
            self.cpu_rms, self.cpu_max, self.max_count = T.rms(cpu), float(cpu.max()), int(cnt.max())
            self.seq32 = T.sequential32(v, idx, n).to(dev) if need_sequential else None

    def check(self, got, label, sorted_form=False):
        if self.any_untouched:
            assert int(torch.count_nonzero(got.view(torch.int32)[self.untouched])) == 0, (label, "untouched targets are not +0.0")
        if self.exact_eq:
            bad = int((got != self.want32).sum())
            assert bad == 0 and torch.equal(got, self.want32), (label, "%d sums differ from float64" % bad)
            return None
        err = (got.double() - self.want).abs()
        over = int((err > self.bound).sum())
        assert over == 0, (label, "%d targets beyond gamma_k sum|x|, worst %g x" % (over, float((err / self.bound)[err > self.bound].max())))
        if sorted_form:
            assert torch.equal(got, self.seq32), (label, "not the ascending-position fp32 sum")
        if self.dist not in ("uniform", "clustered"):
            return None
        gpu_rms, gpu_max = T.rms(err), float(err.max())
        if self.cpu_rms == 0.0:             # at most two contributions anywhere (CPU test): every order gives the same bits
            assert self.max_count <= 2 and gpu_rms == 0.0, (label, gpu_rms)
            return (label, 0.0, 0.0)
        ratio = gpu_rms / self.cpu_rms
        worst = gpu_max / self.cpu_max
        assert ratio <= T.RMS_MARGIN, (label, "RMS error %g = %.2f x the CPU's fp32 index_add_" % (gpu_rms, ratio))
        return (label, worst, ratio)


def _report(case, rows):
    rows = [r for r in rows if r is not None]
    if rows:
        print("\n%s: error over the CPU's fp32 index_add_ (worst, RMS): max %.2f %.2f | %s"
              % (T.case_id(case), max(r[1] for r in rows), max(r[2] for r in rows),
                 "  ".join("%s %.2f %.2f" % r for r in rows)))


@contextlib.contextmanager
def _det(flag):
    """``pointnet2_utils.deterministic_grads(flag)`` for the block; the setting found (None: environment) comes back after."""
    before = PU._DETERMINISTIC
    PU.deterministic_grads(flag)
    try:
        yield
    finally:
        PU._DETERMINISTIC = before


@pytest.mark.parametrize("case", T.GROUP_CASES, ids=T.case_id)
def test_group_points_grad_every_form(cuda, case):
    b, c, n, s, k = case[:5]
    plan = E.group_points_grad_plan(b, c, n, s * k, aligned=True)
    assert T.group_form(plan, c) == case.want, plan
    assert plan["ranges"] == case.opts.get("ranges", plan["ranges"] if plan["form"] == "atomic" else 1), plan
    rows = []
    for dist in T.distributions(case):
        idx = T.make_idx(case, dist)
        idx_d = idx.view(b, s, k).to(cuda)
        assert idx_d.data_ptr() % 16 == 0
        for kind in T.kinds(case):
            v, v64, _ = T.make_values(case, kind, dist)
            R = Ref(v, v64, idx, n, cuda, kind, dist, need_sequential=True)
            go = v.view(b, c, s, k).to(cuda)
            stack = torch.cat((torch.ones(b, 3, s, k, device=cuda), go), dim=1)       # the gradient as channels 3.. of a wider one
            assert go.data_ptr() % 16 == 0 and stack.data_ptr() % 16 == 0
            for det in (False, True):
                with _det(det):
                    outs = []
                    for rep in range(2 if det else 1):
                        feat = torch.zeros(b, c, n, device=cuda, requires_grad=True)
                        PU.grouping_operation(feat, idx_d).backward(go)
                        outs.append(feat.grad)
                        feat = torch.zeros(b, c, n, device=cuda, requires_grad=True)
                        PU.group_concat(idx_d, ("t", torch.zeros(b, 3, s, k, device=cuda)), ("g", feat)).backward(stack)
                        outs.append(feat.grad)
                    tag = "%s/%s/%s" % (dist, kind, "sorted" if det else case.want[0])
                    rows.append(R.check(outs[0], tag + "/dense", sorted_form=det))
                    rows.append(R.check(outs[1], tag + "/strided", sorted_form=det))
                    if det:
                        assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3]), (tag, "differs from run to run")
    _report(case, rows)


MISALIGNED = [c for c in T.GROUP_CASES if (c.b, c.c, c.n, c.s, c.k) in ((32, 64, 64, 37, 4), (128, 9, 64, 37, 4), (1, 1, 64, 2049, 4),
                                                                         (16, 32, 16384, 37, 4))]


@pytest.mark.parametrize("case", MISALIGNED, ids=T.case_id)
@pytest.mark.parametrize("which", ["grad", "idx"])
def test_group_points_grad_misaligned_pointer_takes_scalar_loads(cuda, case, which):
    """P % 4 == 0 but the gradient (or the index list) starts one float into a larger buffer: the launcher reads that off
    the pointer and must not pick the 16-byte loads (the query says so for ``aligned=False``); integer values, so the sums
    are those of float64 bit for bit."""
    b, c, n, s, k = case[:5]
    assert len(MISALIGNED) == 4 and (s * k) % 4 == 0 and case.want[3] == 1
    plan = E.group_points_grad_plan(b, c, n, s * k, aligned=False)
    assert T.group_form(plan, c) == case.want[:3] + (0,) + case.want[4:], plan
    for dist in ("uniform", "last"):
        idx = T.make_idx(case, dist)
        v, v64, _ = T.make_values(case, "int", dist)
        R = Ref(v, v64, idx, n, cuda, "int", dist, need_sequential=False)
        go, idx_d = v.view(b, c, s, k).to(cuda), idx.view(b, s, k).to(cuda)
        if which == "grad":
            buf = torch.zeros(go.numel() + 1, device=cuda)
            buf[1:].copy_(go.reshape(-1))
            go = buf[1:].view(b, c, s, k)
        else:
            buf = torch.zeros(idx_d.numel() + 1, dtype=torch.int32, device=cuda)
            buf[1:].copy_(idx_d.reshape(-1))
            idx_d = buf[1:].view(b, s, k)
        assert (go.data_ptr() % 16, idx_d.data_ptr() % 16) == ((4, 0) if which == "grad" else (0, 4))
        assert go.is_contiguous() and idx_d.is_contiguous()
        R.check(E.group_points_grad(go, idx_d, n), "%s/int/misaligned %s" % (dist, which))


@pytest.mark.parametrize("case", T.INTERP_CASES, ids=T.case_id)
def test_three_interpolate_grad_every_form(cuda, case):
    b, c, n, m = case[:4]
    plan = E.three_interpolate_grad_plan(b, c, n, m)
    assert T.interp_form(plan, c) == case.want, plan
    assert plan["ranges"] == case.opts.get("ranges", plan["ranges"] if plan["form"] == "atomic" else 1), plan
    rows = []
    for dist in T.distributions(case):
        idx = T.make_idx(case, dist)
        idx_d = idx.view(b, n, 3).to(cuda)
        for kind in T.kinds(case):
            v, v64, (g, w) = T.make_values(case, kind, dist)
            R = Ref(v, v64, idx, m, cuda, kind, dist, need_sequential=False)
            got = E.three_interpolate_grad(g.to(cuda), idx_d, w.to(cuda), m)
            rows.append(R.check(got, "%s/%s/%s" % (dist, kind, case.want[0])))
    _report(case, rows)


@pytest.mark.parametrize("case", T.GATHER_CASES, ids=T.case_id)
def test_gather_points_grad_every_form(cuda, case):
    b, c, n, m = case[:4]
    if n * 4 <= 128 * 1024:             # group_points_grad's dispatch with one sample per centre
        assert T.group_form(E.group_points_grad_plan(b, c, n, m, aligned=True), c) == case.want
    else:
        assert case.want == ("gather",)
    rows = []
    for dist in T.distributions(case):
        idx = T.make_idx(case, dist)
        idx_d = idx.to(cuda)
        for kind in T.kinds(case):
            v, v64, _ = T.make_values(case, kind, dist)
            R = Ref(v, v64, idx, n, cuda, kind, dist, need_sequential=True)
            go = v.to(cuda)
            for det in (False, True):
                with _det(det):
                    feat = torch.zeros(b, c, n, device=cuda, requires_grad=True)
                    PU.gather_operation(feat, idx_d).backward(go)
                tag = "%s/%s/%s" % (dist, kind, "sorted" if det else case.want[0])
                rows.append(R.check(feat.grad, tag, sorted_form=det))
                if det:
                    assert torch.equal(feat.grad, E.scatter_grad_deterministic(go, idx_d, n)), (tag, "differs from run to run")
                else:
                    R.check(E.gather_points_grad(go, idx_d, n), tag + "/ext")
    _report(case, rows)


# ---- geometry_encode_grad, broadcast_centre_grad, xyz_diff backward ------------------------------------------------------
def _chain(cx, sx, pf, idx, k):
    """The reference's torch ops for the parts ("geo", cx, sx), ("c", pf), ("diff", cx, sx) (PW/costvolume.py:92-105,
    P2/pointnet2_modules.py:215-218), in the dtype of the arguments."""
    s = cx.shape[2]
    gather = lambda t: torch.gather(t.unsqueeze(2).expand(-1, -1, s, -1), 3,
                                    idx.to(t.device).long().unsqueeze(1).expand(-1, t.shape[1], -1, -1))
    q = gather(sx)
    p = cx.unsqueeze(3).expand(-1, -1, -1, k)
    diff = q - p
    euc = torch.sqrt(torch.sum(torch.square(diff), dim=1, keepdim=True) + 1e-20)
    return torch.cat((p, q, diff, euc), dim=1), pf.unsqueeze(3).expand(-1, -1, -1, k), gather(sx) - p


@pytest.mark.parametrize("k", [1, 3, 4, 6, 32])
def test_geometry_broadcast_and_diff_gradients_on_a_lattice(cuda, k):
    """Centres and sources on an integer lattice (differences exact), centres among the sources and every centre its own
    first neighbour (q == p: |q - p| = sqrt(1e-20), the norm channel sends nothing back), integer gradients.  Dense (the
    part is the whole tensor) and as slices of a wider gradient at channel offsets 1, 11 and 16; s = 300 is no multiple of
    the 256-thread block.  (Every such slice of a torch tensor is 16-byte aligned when k % 4 == 0, so
    broadcast_centre_grad's scalar loads are reached through k = 1, 3, 6 and its 16-byte ones through k = 4, 32.)
    broadcast_centre_grad and both sides of xyz_diff add integers: equal to float64.
    geometry_encode_grad divides by the norm: per element within gamma_(count + 10) * sum |term| of float64 (at most five
    roundings per pair -- sqrt, quotient, product, two adds -- then the sum), atomics and sorted scatter alike."""
    b, n, s, cf = 2, 400, 300, 5
    gen = torch.Generator().manual_seed(1000 + k)
    src = torch.randint(-3, 4, (b, 3, n), generator=gen).float()
    centre = src[:, :, :s].clone()
    idx = torch.randint(0, n, (b, s, k), generator=gen, dtype=torch.int32)
    idx[:, :, 0] = torch.arange(s, dtype=torch.int32)
    pf = torch.randint(-8, 9, (b, cf, s), generator=gen).float()
    go = torch.randint(-8, 9, (b, 1 + 10 + cf + 3, s, k), generator=gen).float()
    idx_d = idx.to(cuda)

    l64 = [t.double().requires_grad_(True) for t in (centre, src, pf, centre, src)]
    geo64, c64, d64 = _chain(l64[0], l64[1], l64[2], idx, k)
    geo64.backward(go[:, 1:11].double())
    c64.backward(go[:, 11:11 + cf].double())
    (l64[4].unsqueeze(2).expand(-1, -1, s, -1).gather(3, idx.long().unsqueeze(1).expand(-1, 3, -1, -1))
     - l64[3].unsqueeze(3)).backward(go[:, 11 + cf:].double())
    # sum of |term| per element for the geometry gradients
    q = torch.gather(src.double().unsqueeze(2).expand(-1, -1, s, -1), 3, idx.long().unsqueeze(1).expand(-1, 3, -1, -1))
    diff = q - centre.double().unsqueeze(3)
    euc = torch.sqrt(diff.pow(2).sum(1, keepdim=True) + 1e-20)
    g = go[:, 1:11].double().abs()
    norm_part = g[:, 9:10] * diff.abs() / euc
    mag_c = (g[:, 0:3] + g[:, 6:9] + norm_part).sum(3)
    pair = (g[:, 3:6] + g[:, 6:9] + norm_part).reshape(b, 3, s * k)
    ix = idx.long().reshape(b, 1, s * k).expand(-1, 3, -1)
    mag_s = torch.zeros(b, 3, n, dtype=torch.float64).scatter_add_(2, ix, pair)
    cnt_s = torch.zeros(b, 3, n, dtype=torch.float64).scatter_add_(2, ix, torch.ones_like(pair))

    def run(det, sliced, grad=go):
        leaves = [t.to(cuda).requires_grad_(True) for t in (centre, src, pf, centre, src)]
        with _det(det):
            if sliced:
                out = PU.group_concat(idx_d, ("t", torch.zeros(b, 1, s, k, device=cuda)), ("geo", leaves[0], leaves[1]),
                                      ("c", leaves[2]), ("diff", leaves[3], leaves[4]))
                out.backward(grad.to(cuda))
            else:
                PU.group_concat(idx_d, ("geo", leaves[0], leaves[1])).backward(grad[:, 1:11].contiguous().to(cuda))
                PU.group_concat(idx_d, ("c", leaves[2])).backward(grad[:, 11:11 + cf].contiguous().to(cuda))
                PU.group_concat(idx_d, ("diff", leaves[3], leaves[4])).backward(grad[:, 11 + cf:].contiguous().to(cuda))
        return [t.grad.cpu() for t in leaves]

    for det in (False, True):
        for sliced in (False, True):
            dc, ds, dpf, dc2, ds2 = run(det, sliced)
            tag = (k, det, sliced)
            assert torch.equal(dpf.double(), l64[2].grad), tag                         # broadcast_centre_grad
            assert torch.equal(dc2.double(), l64[3].grad) and torch.equal(ds2.double(), l64[4].grad), tag      # xyz_diff
            assert bool(((dc.double() - l64[0].grad).abs() <= T.gamma(k + 10) * mag_c).all()), tag
            assert bool(((ds.double() - l64[1].grad).abs() <= T.gamma(cnt_s + 10) * mag_s).all()), tag
            assert int(torch.count_nonzero(ds.view(torch.int32)[cnt_s == 0])) == 0, tag      # untouched sources: +0.0

    # every pair q == p and a gradient on the norm channel alone: float64 sends back exactly zero, and so must the kernel
    own = torch.arange(s, dtype=torch.int32).view(1, s, 1).expand(b, s, k).contiguous()
    norm_only = torch.zeros(b, 10, s, k)
    norm_only[:, 9] = go[:, 10]
    c64n, s64n = centre.double().requires_grad_(True), src.double().requires_grad_(True)
    _chain(c64n, s64n, pf.double(), own, k)[0].backward(norm_only.double())
    assert not c64n.grad.any() and not s64n.grad.any()
    for det in (False, True):
        cx, sx = centre.to(cuda).requires_grad_(True), src.to(cuda).requires_grad_(True)
        with _det(det):
            PU.group_concat(own.to(cuda), ("geo", cx, sx)).backward(norm_only.to(cuda))
        assert torch.equal(cx.grad.cpu().double(), c64n.grad) and torch.equal(sx.grad.cpu().double(), s64n.grad), (k, det)

    # Inf / NaN on the norm channel, at q == p pairs (column 0) and elsewhere: where torch's own fp32 expression of the chain
    # gives NaN or an infinity, so does the kernel, and nowhere else
    special = go[:, 1:11].clone()
    vals = torch.tensor([float("inf"), float("-inf"), float("nan"), 1e30, 1e28])
    cols = [0] if k == 1 else [0, k - 1]
    for j in range(0, s, 7):
        special[j % b, 9, j, cols[(j // 7) % len(cols)]] = vals[(j // 7) % len(vals)]
    ct, st = centre.to(cuda).requires_grad_(True), src.to(cuda).requires_grad_(True)
    _chain(ct, st, pf.to(cuda), idx, k)[0].backward(special.to(cuda))
    for det in (False, True):
        cx, sx = centre.to(cuda).requires_grad_(True), src.to(cuda).requires_grad_(True)
        with _det(det):
            PU.group_concat(idx_d, ("geo", cx, sx)).backward(special.to(cuda))
        for got, want in ((cx.grad, ct.grad), (sx.grad, st.grad)):
            assert torch.equal(torch.isnan(got), torch.isnan(want)), (k, det)
            assert torch.equal(torch.isinf(got) * torch.sign(got).nan_to_num(0), torch.isinf(want) * torch.sign(want).nan_to_num(0)), (k, det)
        assert bool(torch.isnan(ct.grad).any())
