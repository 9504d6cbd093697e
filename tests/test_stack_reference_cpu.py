"""tests/stack_reference.py on the CPU: the model is pinned to the oracle (which is pinned to the reference), the two
criteria of tests/test_gpu_stack_variants.py reject subtly wrong kernels (CPU stand-ins), and the inputs of every bf16
row of that file's table leave its bound alone."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stack_reference as SR                                                     # noqa: E402
import stack_cases as V                                                          # noqa: E402
from oracle import model as M                                                    # noqa: E402
from oracle import ops as O                                                      # noqa: E402

pm = lambda t: t.permute(0, 2, 1).contiguous()      # (B,C,N) <-> (B,N,C)


def osd(module, prefix):
    return {prefix + "." + k: v.clone() for k, v in module.state_dict().items()}


def close(a, b):
    assert SR.close_1e5(a, b) == 0, "max abs err %.3e (scale %.3e)" % ((a - b).abs().max().item(), b.abs().max().item())


E32 = dict(rounding=SR.EXACT, dtype=torch.float32)


@pytest.mark.parametrize("name,mlp,npoint,nsample,n", [("psa_1", [0, 8, 8, 16], 64, 20, 300),
                                                        ("psa_3", [32, 32, 32, 64], 37, 11, 301)])
def test_model_in_fp32_is_the_oracles_set_abstraction(name, mlp, npoint, nsample, n):
    mod = V.filled(V.PointnetSAModulePWCLONet(mlp=list(mlp), npoint=npoint, nsample=nsample), name)
    xyz, feat = V.cloud(1, 2, n), (V.randn(2, 2, mlp[0], n) if mlp[0] else None)
    ref_xyz, ref = M.set_abstraction(osd(mod, name), name, npoint, nsample, xyz, feat)
    idx = O.knn_point_with_dist(nsample, xyz, ref_xyz)[1]
    got = SR.set_abstraction(mod, xyz, ref_xyz, pm(feat) if feat is not None else None, idx, **E32)
    close(pm(got), ref)


def test_model_in_fp32_is_the_oracles_set_upconv_and_flow_predictor():
    name = "pose_warp_refinement_2.setupconv_features"
    mod = V._upconv_module(name, 32)
    xyz2, xyz1, f2, f1 = V.cloud(3, 2, 333), V.cloud(4, 2, 90), V.randn(5, 2, 32, 333), V.randn(6, 2, 64, 90)
    ref = M.set_upconv(osd(mod, name), name, 8, xyz2, xyz1, f2, f1)
    idx = O.knn_point_with_dist(8, xyz1, xyz2)[1]
    close(pm(SR.set_upconv(mod, xyz2, xyz1, pm(f2), pm(f1), idx, **E32)), ref)
    fp = V.filled(V.FlowPredictor(in_channel=160, mlp=[128, 64]), "l4_flow_predictor")
    srcs = [V.randn(7 + i, 2, c, 203) for i, c in enumerate((32, 64, 64))]
    ref = M.flow_predictor(osd(fp, "l4_flow_predictor"), "l4_flow_predictor", *srcs)
    close(pm(SR.pointwise(fp.mlp_convs, [pm(s) for s in srcs], **E32)), ref)


@pytest.mark.parametrize("kq,c,s,n", [(6, 16, 301, 280), (20, 64, 70, 90)])
def test_model_in_fp32_is_the_oracles_cost_volume(kq, c, s, n):
    mod = V.filled(V.CostVolume(nsample=4, nsample_q=kq, in_channel1=c, in_channel2=c, mlp1=[128, 64, 64],
                                mlp2=[128, 64]), "cost_volume")
    x1, x2, p1, p2 = pm(V.cloud(7, 2, s)), pm(V.cloud(8, 2, n)), V.randn(9, 2, c, s), V.randn(10, 2, c, n)
    taps = {}
    ref = M.cost_volume(osd(mod, "cost_volume"), "cost_volume", 4, kq, x1, p1, x2, p2, taps, "cv")
    out, first = SR.cost_volume(mod, pm(x1), pm(p1), pm(x2), pm(p2), taps["cv.idx_q"], taps["cv.idx"], **E32)
    close(pm(first), taps["cv.first"])
    close(pm(out), ref)


# ---- the criteria can fail -------------------------------------------------------------------------------------------

def _bf16_stand_in(**wrong):
    """Flow-feature encoding (67 -> 128 -> 64 -> 64: two bf16 layers behind bf16 seed rows) on the table's inputs: the
    figures of the bf16 criterion with the float64 model evaluated WRONGLY (``wrong``) standing in for the kernel."""
    case = next(c for c in V.CASES if c.kind == "sa" and c.fmt == V.B16 and c.name == "flow_feature_encoding" and c.s == 683)
    i = V.inputs_of(case)
    got = case.model(i, rounding=SR.BF16, dtype=torch.float32, **wrong)
    ex, m64, m32 = (V.reference(case, r, d) for r, d in ((SR.EXACT, torch.float64), (SR.BF16, torch.float64),
                                                         (SR.BF16, torch.float32)))
    return SR.bf16_figures(got[0], ex[0], m64[0], m32[0])


def test_bf16_criterion_rejects_truncation_and_a_missing_rounding_point():
    right = _bf16_stand_in()
    assert not SR.bf16_violations(right) and SR.inputs_clear_of_bound(right), right
    trunc = _bf16_stand_in(round_fn=SR.round_truncate)
    print("\ntruncation: R / Ebf = %.2f (correct: %.3f)" % (trunc["r"] / trunc["ebf"], right["r"] / right["ebf"]))
    assert trunc["r"] > trunc["ebf"] / 8
    # layer 3 computed from unrounded activations (its weights still bf16)
    skipped = _bf16_stand_in(skip_input=("l3",))
    print("input rounding of one layer left out: R / Ebf = %.2f" % (skipped["r"] / skipped["ebf"]))
    assert skipped["r"] > skipped["ebf"] / 8


def _split3(x):
    hi = x.to(torch.bfloat16).float()
    mid = (x - hi).to(torch.bfloat16).float()
    return hi, mid, (x - hi - mid).to(torch.bfloat16).float()


def _split_layer(x, w, b, drop_hi_lo):
    """csrc/mlp_core.hpp mlp_layer_bf3_init in plain fp32: six of the nine cross products of the three-term splits."""
    (xh, xm, xl), (wh, wm, wl) = _split3(x), _split3(w)
    terms = [(wl, xh), (wh, xl), (wm, xm), (wm, xh), (wh, xm), (wh, xh)]
    if drop_hi_lo:
        del terms[1]
    acc = b.expand(x.shape[0], -1).clone()
    for w_, x_ in terms:
        acc = acc + x_ @ w_.t()
    return torch.relu(acc)


def test_fp32_criterion_rejects_a_split_layer_without_its_hi_lo_product():
    x = V.randn(1, 4096, 128)
    ws = [(V.randn(2, 128, 128) / 128 ** 0.5, V.randn(3, 128) * 0.1), (V.randn(4, 64, 128) / 128 ** 0.5, V.randn(5, 64) * 0.1)]
    ev = lambda dt: torch.relu(torch.relu(x.to(dt) @ ws[0][0].to(dt).t() + ws[0][1].to(dt)) @ ws[1][0].to(dt).t() + ws[1][1].to(dt))
    exact, e32 = ev(torch.float64), ev(torch.float32)
    for drop in (False, True):
        got = _split_layer(_split_layer(x, *ws[0], drop), *ws[1], drop)
        f = SR.fp32_figures(got, exact, e32)
        print("\nsplit stack, hi.lo %s: max %.2f x E32, rms %.2f x E32, %d outside 1e-5" % (
            "dropped" if drop else "kept", f["k_max"] / f["e32_max"], f["k_rms"] / f["e32_rms"], f["outside_1e5"]))
        if drop:
            assert f["outside_1e5"] == 0                                 # the suite's bound cannot see it ...
            assert f["k_max"] > 4 * f["e32_max"] and f["k_rms"] > 4 * f["e32_rms"]      # ... the 4 x E32 bound does
        else:
            assert not SR.fp32_violations(f), f


BF16_ROWS = [c for c in V.CASES if c.fmt == V.B16]


@pytest.mark.parametrize("case", BF16_ROWS, ids=[c.id for c in BF16_ROWS])
def test_inputs_of_every_bf16_row_stay_clear_of_the_bound(case):
    """R <= Ebf / 8 is a condition on the inputs as well: 4 x R_ref <= Ebf / 8 on the CPU for every bf16 row (rows whose
    stack has no rounding point -- Ebf = 0 -- are judged by the fp32 criterion instead)."""
    for f in V.bf16_row_figures(case):
        print("\n%s: Ebf %.3e  R_ref %.3e  (Ebf / 8) / R_ref = %.1f" % (case.want, f["ebf"], f["r_ref"],
                                                                       f["ebf"] / 8 / max(f["r_ref"], 1e-300)))
        if f["ebf"] == 0:
            assert f["model_max"] == 0
        else:
            assert SR.inputs_clear_of_bound(f), f
