"""Float64 host model of the fused stack layers, with a model of where the bf16 format rounds (a test helper: not a
conftest, not a product module).

Written from the modules' mathematics (oracle/model.py states the same layers on (B,C,S,K) tensors), not from the
kernels: conv + eval-mode BatchNorm folded here in float64, neighbour lists given, activations point-major (B,N,C).
Every function takes

* ``rounding``: "exact" (no rounding point) or "bf16" (round to nearest even where the bf16 format rounds), and
* ``dtype``: torch.float64 or torch.float32, the type every product and sum is carried out in.

("exact", float64) is the reference; ("exact", float32) is the CPU's own fp32 error on the same inputs, the yardstick
of the fp32-accurate kernels (fp32 and bf16x3 tiles); ("bf16", float64) is what a correct bf16 kernel computes up to
fp32 accumulation, and ("bf16", float32) shows how far fp32 accumulation alone moves that (an activation next to a
rounding boundary rounds the other way).

Rounding points of ``"bf16"`` and where each comes from
-------------------------------------------------------
1. Weights of a layer with an even number of 16-channel input blocks: rounded once when packed
   (pwclonet_pylidarslam_amd/fused.py ``pack_layer``: ``hi = wt.to(torch.bfloat16)``, taken when
   ``layer_wfmt(wfmt, nbi)`` is not fp32).
2. Input activations of the same layers: rounded when the layer starts (csrc/mlp_core.hpp ``mlp_layer_bf16_init``:
   ``x[mp][p] = to_bf16x8(in[2 * mp][p], in[2 * mp + 1][p])``; ``mlp_layer_any`` sends only ``NBI % 2 == 0`` there).
3. Layers with an odd number of input blocks stay fp32: the lone geometry blocks (diff(3), [diff, xyz](6),
   geometry(10)), every layer of psa_1 (6 -> 8 -> 8 -> 16) and of psa_2 (16 -> 16 -> 32 after hoisting)
   (``fused.layer_wfmt``, the predicate ``pack_layer`` itself uses).
4. Biases, hoisted seeds and accumulation: never rounded (``mlp_layer_bf16_init`` seeds ``acc[p] = init(o, p)`` in fp32
   and accumulates with v_mfma_f32_16x16x32_bf16).
5. Hoisted rows (the outputs of ``LinearJob(out_bf16=True)``: set-abstraction and set-upconv seeds, the cost volume's
   u, v, u2, v2): computed with fp32 weights, rounded once when stored (csrc/fused_hoisted.hip ``linear_tiles``:
   ``st_group<true>``; csrc/mlp_core.hpp ``st4_bf16``), read back exactly (``ld_group<true>`` / ``ld4_bf16``).
   ``fused.py`` sets ``out_bf16`` where the consumer's format is bf16 (FusedSAHoisted, FusedUpconvHoisted,
   FusedCostVolumeHoisted ``h16``).
6. The cost volume's per-pixel buffer between cv_a1_h and cv_a2: rounded once when stored (csrc/fused_hoisted.hip
   ``cv_a1_h_kernel``: ``st_group<H16>(a.out, ...)``), read back exactly (csrc/fused_layers.hip ``load_pix_blocks``);
   the soft-max weights multiply the stored (rounded) features.
7. A cost volume whose first aggregate has 8 or 16 pixel slots runs fp32 whatever was asked for, and the un-hoisted
   cost volume never stores bf16 (``fused.cv_stack_wfmt``, the predicate both cost-volume classes use).
8. The point-wise stacks (``FusedPointwise``, with or without the linear tail) and the un-hoisted set abstraction and
   set-upconv pack fp32 tiles whatever the format: no rounding point.
9. Coordinates, differences, distances, the soft-max and the pooling are never rounded.
"""
import math

import torch

from pwclonet_pylidarslam_amd import fused

EXACT, BF16 = "exact", "bf16"


def round_nearest(x):
    """Round to the nearest bf16 (ties to even), result in x's type."""
    return x.to(torch.bfloat16).to(x.dtype)


def round_truncate(x):
    """The WRONG rounding (drop the low 16 bits of the fp32 pattern): only for showing that the criteria notice it."""
    f = x.to(torch.float32).contiguous()
    return (f.view(torch.int32) & -65536).view(torch.float32).to(x.dtype)


class _R:
    """One evaluation's arithmetic: the type, the rounding function and the stack's tile format.  ``round_fn`` and
    ``skip_input`` (names of layers whose input rounding is left out) exist for the sensitivity checks only."""

    def __init__(self, rounding, dtype, round_fn=None, skip_input=()):
        assert rounding in (EXACT, BF16) and dtype in (torch.float64, torch.float32)
        self.dtype = dtype
        self.fmt = fused.WFMT_BF16 if rounding == BF16 else fused.WFMT_F32
        self.fn = round_fn or round_nearest
        self.skip_input = set(skip_input)

    def cast(self, *ts):
        out = tuple(None if t is None else t.detach().cpu().to(self.dtype) for t in ts)
        return out[0] if len(out) == 1 else out

    def store(self, x, fmt=None):
        """A row buffer written by a kernel of format ``fmt``: bf16 rows exactly when that format is bf16."""
        return self.fn(x) if (self.fmt if fmt is None else fmt) == fused.WFMT_BF16 else x

    def layer(self, x, w, b, relu=True, seed=None, fmt=None, name=None):
        """relu(x . w^T + b) over the last axis (``seed``: per-row accumulator seed used instead of the bias)."""
        nbi = (x.shape[-1] + 15) // 16
        if fused.layer_wfmt(self.fmt if fmt is None else fmt, nbi) == fused.WFMT_BF16:
            w = self.fn(w)
            if name not in self.skip_input:
                x = self.fn(x)
        y = x @ w.t() + (b if seed is None else seed)
        return torch.relu(y) if relu else y


def fold(layer, dtype=torch.float64):
    """One SharedMLP entry (conv [+ bn]) -> (W (Cout,Cin), bias (Cout,)) of the eval-mode affine map, folded in
    float64 and then cast to ``dtype``."""
    conv = layer.conv
    w = conv.weight.detach().cpu().double().reshape(conv.weight.shape[0], -1)
    b = conv.bias.detach().cpu().double() if conv.bias is not None else torch.zeros(w.shape[0], dtype=torch.float64)
    if hasattr(layer, "bn"):
        bn = layer.bn.bn
        s = bn.weight.detach().cpu().double() / torch.sqrt(bn.running_var.detach().cpu().double() + bn.eps)
        w = w * s[:, None]
        b = (b - bn.running_mean.detach().cpu().double()) * s + bn.bias.detach().cpu().double()
    return w.to(dtype), b.to(dtype)


def rows(t, idx):
    """t (B,N,C), idx (B,S,K) -> (B,S,K,C)."""
    return t[torch.arange(t.shape[0])[:, None, None], idx.long()]


def _geometry10(p, q):
    """p (B,S,3) centres, q (B,S,K,3) neighbours -> [p, q, q - p, |q - p|] (B,S,K,10)."""
    pc = p[:, :, None, :].expand_as(q)
    d = q - pc
    euc = torch.sqrt((d * d).sum(-1, keepdim=True) + 1e-20)
    return torch.cat((pc, q, d, euc), dim=-1)


def linear_job(w, b, src, out_bf16=False, rounding=EXACT, dtype=torch.float64, **kw):
    """A lone ``LinearJob``: src . w^T + b with fp32 weights, the rows rounded when stored as bf16."""
    r = _R(rounding, dtype, **kw)
    w, b, src = r.cast(w, b, src)
    return r.store(src @ w.t() + b, fused.WFMT_BF16 if out_bf16 and rounding == BF16 else fused.WFMT_F32)


def pointwise(shared_mlp, sources, tail=None, rounding=EXACT, dtype=torch.float64, **kw):
    """``FusedPointwise``: the SharedMLP over cat(sources); ``tail`` = (w, b) of a linear layer on its output ->
    (out, tail rows).  fp32 tiles in every format: no rounding point."""
    r = _R(EXACT, dtype)
    x = torch.cat(r.cast(*sources) if len(sources) > 1 else (r.cast(*sources),), dim=-1)
    for layer in shared_mlp:
        x = r.layer(x, *fold(layer, dtype))
    if tail is None:
        return x
    w, b = r.cast(*tail)
    return x, x @ w.t() + b


def set_abstraction(module, xyz, new_xyz, feat, idx, rounding=EXACT, dtype=torch.float64, **kw):
    """``PointnetSAModulePWCLONet`` on given samples and lists: xyz (B,N,3), new_xyz (B,S,3), feat (B,N,C) or None,
    idx (B,S,K) -> (B,S,Cout).  The bf16 model is the hoisted kernel's (the un-hoisted one has fp32 tiles only)."""
    r = _R(rounding, dtype, **kw)
    (w1, b1), (w2, b2), (w3, b3) = [fold(l, dtype) for l in module.mlp_module]
    xyz, new_xyz, feat = r.cast(xyz, new_xyz, feat)
    q = rows(xyz, idx)
    diff = q - new_xyz[:, :, None, :]
    if feat is None:
        h = r.layer(torch.cat((diff, q), dim=-1), w1, b1)                       # [xyz_diff, grouped_xyz]
    else:
        pre = r.store(feat @ w1[:, 3:].t() + b1)                                # [xyz_diff(3) | feat]: hoisted rows
        h = r.layer(diff, w1[:, :3], None, seed=rows(pre, idx))
    h = r.layer(h, w2, b2, name="l2")
    h = r.layer(h, w3, b3, relu=False, name="l3")
    return torch.relu(h.max(dim=2).values)


def set_upconv(module, xyz2, xyz1, feat2, feat1, idx, post=True, rounding=EXACT, dtype=torch.float64, **kw):
    """``PointnetFPModulePWCLONet`` (knn branch): xyz2 (B,S,3) fine, xyz1 (B,N,3) coarse, feat2 (B,S,C2),
    feat1 (B,N,64), idx (B,S,K) -> (B,S,64); ``post=False``: the pooled rows before the post-MLP."""
    r = _R(rounding, dtype, **kw)
    (w1, b1), (w2, b2) = [fold(l, dtype) for l in module.mlp]
    xyz2, xyz1, feat1 = r.cast(xyz2, xyz1, feat1)
    pre = r.store(feat1 @ w1[:, :64].t() + b1)                                  # [feat(64) | xyz_diff(3)]
    diff = rows(xyz1, idx) - xyz2[:, :, None, :]
    h = r.layer(diff, w1[:, 64:], None, seed=rows(pre, idx))
    h = r.layer(h, w2, b2, relu=False, name="l2")
    pooled = torch.relu(h.max(dim=2).values)
    if not post:
        return pooled
    return pointwise(module.post_mlp, [pooled, feat2], dtype=dtype)


def cost_volume(module, xyz1, feat1, xyz2, feat2, idx_q, idx, hoisted=True, rounding=EXACT, dtype=torch.float64, **kw):
    """``CostVolume``: xyz1 (B,S,3) warped frame-1 points, feat1 (B,S,C), xyz2 (B,N,3), feat2 (B,N,C), idx_q (B,S,Kq)
    among frame 2, idx (B,S,K) among frame 1 -> (out (B,S,64), first (B,S,64)): both aggregates, each a soft-max
    over its neighbours."""
    r = _R(rounding, dtype, **kw)
    c = module.in_channel[0]
    fmt = fused.cv_stack_wfmt(fused.cv_pix_slots(module.nsample_q), r.fmt, hoisted=hoisted)     # point 7
    xyz1, feat1, xyz2, feat2 = r.cast(xyz1, feat1, xyz2, feat2)
    (w1, b1), (w2, b2), (w3, b3) = [fold(l, dtype) for l in module.mlp_convs]   # [geo(10) | feat1 | feat2]
    (wx1, bx1), = [fold(l, dtype) for l in module.mlp_conv_xyz_1]
    (wa, ba), (wb, bb) = [fold(l, dtype) for l in module.mlp2_convs]            # [enc | feat]
    (wx2, bx2), = [fold(l, dtype) for l in module.mlp_conv_xyz_2]
    (wc, bc), (wd, bd) = [fold(l, dtype) for l in module.mlp3_convs]            # [enc2 | feat1 | first]

    geo = _geometry10(xyz1, rows(xyz2, idx_q))
    u = r.store(feat1 @ w1[:, 10:10 + c].t() + b1, fmt)
    v = r.store(feat2 @ w1[:, 10 + c:].t(), fmt)
    h = r.layer(geo, w1[:, :10], None, seed=u[:, :, None, :] + rows(v, idx_q), fmt=fmt)
    h = r.layer(h, w2, b2, fmt=fmt, name="a1.l2")
    pix = r.store(r.layer(h, w3, b3, fmt=fmt, name="a1.l3"), fmt)              # the per-pixel buffer
    enc = r.layer(geo, wx1, bx1, fmt=fmt)
    a = r.layer(torch.cat((enc, pix), dim=-1), wa, ba, fmt=fmt, name="a2.l1")
    a = r.layer(a, wb, bb, fmt=fmt, name="a2.l2")
    first = (torch.softmax(a, dim=2) * pix).sum(dim=2)

    geo2 = _geometry10(xyz1, rows(xyz1, idx))
    u2 = r.store(feat1 @ wc[:, 64:64 + c].t() + bc, fmt)
    v2 = r.store(first @ wc[:, 64 + c:].t(), fmt)
    enc2 = r.layer(geo2, wx2, bx2, fmt=fmt)
    g = r.layer(enc2, wc[:, :64], None, seed=u2[:, :, None, :] + rows(v2, idx), fmt=fmt, name="b.l1")
    g = r.layer(g, wd, bd, fmt=fmt, name="b.l2")
    out = (torch.softmax(g, dim=2) * rows(first, idx)).sum(dim=2)
    return out, first


# ---- criteria ------------------------------------------------------------------------------------------------------

def _err(a, b):
    d = (a.detach().cpu().double() - b.detach().cpu().double())
    return d.abs().max().item(), math.sqrt((d * d).mean().item())


def close_1e5(a, b, rel=1e-5):
    """The suite's mixed bound |a - b| <= 1e-5 |b| + 1e-5 max|b| -> number of elements outside it."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return int(((a - b).abs() > rel * b.abs() + rel * b.abs().max()).sum())


def fp32_figures(got, exact64, exact32):
    """Figures of the fp32 criterion.  E32 = the CPU's own fp32 error on the same inputs."""
    e_max, e_rms = _err(exact32, exact64)
    k_max, k_rms = _err(got, exact64)
    return dict(scale=exact64.abs().max().item(), e32_max=e_max, e32_rms=e_rms, k_max=k_max, k_rms=k_rms,
                outside_1e5=close_1e5(got, exact64), finite=bool(torch.isfinite(got).all()))


def fp32_violations(f):
    """The fp32 criterion: max and RMS error against float64 each within 4 x E32 (the margin covers the other summation
    order: MFMA k-steps against torch's blocked dot), and the suite's 1e-5 mixed bound."""
    bad = []
    if not f["finite"]:
        bad.append("not finite")
    if f["k_max"] > 4 * f["e32_max"]:
        bad.append("max error %.3e > 4 x E32(max) %.3e" % (f["k_max"], f["e32_max"]))
    if f["k_rms"] > 4 * f["e32_rms"]:
        bad.append("RMS error %.3e > 4 x E32(rms) %.3e" % (f["k_rms"], f["e32_rms"]))
    if f["outside_1e5"]:
        bad.append("%d elements outside the 1e-5 mixed bound" % f["outside_1e5"])
    return bad


def bf16_figures(got, exact64, model64, model32):
    """Figures of the bf16 criterion.  Ebf = RMS(model - exact): what the format costs; R = RMS(kernel - model): what the
    kernel adds; R_ref = RMS(model in fp32 - model in float64): what fp32 accumulation alone adds on the CPU."""
    m_max, ebf = _err(model64, exact64)
    _, r = _err(got, model64)
    _, r_ref = _err(model32, model64)
    k_max, _ = _err(got, exact64)
    return dict(scale=exact64.abs().max().item(), ebf=ebf, model_max=m_max, r=r, r_ref=r_ref, k_max=k_max,
                finite=bool(torch.isfinite(got).all()))


def bf16_violations(f):
    """The bf16 criterion: R <= Ebf / 8, max |kernel - exact| <= 2 x max |model - exact|, everything finite."""
    bad = []
    if not f["finite"]:
        bad.append("not finite")
    if f["r"] > f["ebf"] / 8:
        bad.append("R %.3e > Ebf / 8 = %.3e" % (f["r"], f["ebf"] / 8))
    if f["k_max"] > 2 * f["model_max"]:
        bad.append("max |kernel - exact| %.3e > 2 x max |model - exact| %.3e" % (f["k_max"], f["model_max"]))
    return bad


def inputs_clear_of_bound(f):
    """Condition on the INPUTS of a bf16 case: the CPU's own residual must sit 4 x below the bound, 4 R_ref <= Ebf / 8."""
    return 4 * f["r_ref"] <= f["ebf"] / 8
