"""The kernels that turn the network's last tensor into the pose, at every form and edge (run with ``-m gpu -s``):
``pose_head_kernel`` and ``masked_pool_kernel`` (csrc/fused_layers.hip) against a float64 evaluation of the reference
formula by the fp32 criterion of tests/stack_reference.py (max and RMS error within 4 x E32, the CPU's own float32 error
on the same inputs, and the 1e-5 mixed bound), ``quat_warp_kernel<false/true>`` (csrc/warp.hip) and the pose head's
in-launch warp bit for bit against the reference's left-to-right expression.  Cases, host models and why each case exists:
tests/pose_cases.py; that the cases catch wrong kernels: tests/test_pose_cases_cpu.py.
"""
import numpy as np
import pytest
import torch

import pose_cases as PC
import stack_reference as SR
from pwclonet_pylidarslam_amd import fused
from pwclonet_pylidarslam_amd.pointnet2_ops import _ext
from pwclonet_pylidarslam_amd.pwclonet import PoseCalculator

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e11     # what pose_params holds before the launch; compared through its bits

pm = lambda t: t.permute(0, 2, 1).contiguous()      # (B,C,N) <-> (B,N,C)
bits = lambda t: t.detach().cpu().contiguous().view(torch.int32)


def _violations(name, got, ex64, ex32):
    """tests/stack_reference.py's fp32 criterion, as it stands, printed like test_gpu_dropout._head_violations.
    -> (violations, max-error ratio to E32, RMS ratio to E32)."""
    f = SR.fp32_figures(got.detach().cpu().reshape(ex64.shape), ex64, ex32)
    ratio = lambda a, b: a / b if b > 0 else (0.0 if a == 0 else float("inf"))
    r_max, r_rms = ratio(f["k_max"], f["e32_max"]), ratio(f["k_rms"], f["e32_rms"])
    print("  %-9s scale %.3g  E32 max %.3e rms %.3e | kernel max %.3e (%.2f x) rms %.3e (%.2f x)"
          % (name, f["scale"], f["e32_max"], f["e32_rms"], f["k_max"], r_max, f["k_rms"], r_rms))
    return ["%s: %s" % (name, v) for v in SR.fp32_violations(f)], r_max, r_rms


@pytest.fixture(scope="module")
def head(cuda):
    pc = PoseCalculator(in_channel=64, out_channel=256, kernel_size=1, padding="valid", activation=None, squeeze=False)
    convs = (pc.conv1d_q_t.conv, pc.conv1d_q.conv, pc.conv1d_t.conv)
    with torch.no_grad():
        for i, w in enumerate(PC.head_weights()):
            (convs[i // 2].weight if i % 2 == 0 else convs[i // 2].bias).copy_(w)
    return fused.FusedPoseHead(pc.eval().to(cuda))


@pytest.mark.parametrize("case", PC.HEAD_CASES, ids=[c.name for c in PC.HEAD_CASES])
def test_pose_head_against_float64(cuda, head, case):
    """q, t and the 7-float row of one launch against the float64 model; with ``warp_next`` the warped cloud is
    bit-identical to ``quat_warp_pm`` and to ``warp_expr`` on the q, t the launch returned; the row holds t bit for bit
    and q normalised; every other float of pose_params keeps its bits; the launch without the warp returns the same bits."""
    x = PC.head_inputs(case)
    (_, q64, t64, row64), (_, q32, t32, row32) = PC.head_reference(case.name)
    dev = lambda v: None if v is None else v.to(cuda)
    emb, logits, q_prev, t_prev, nxt = (dev(x[k]) for k in ("emb", "logits", "q_prev", "t_prev", "warp_next"))
    pose = torch.full((PC.B_HEAD, 4, 7), SENTINEL, device=cuda)
    q, t = head(emb, logits, pose, case.level, q_prev, t_prev)
    row = pose[:, case.level]
    print("\n%s (%s):" % (case.name, case.why))
    bad, worst = [], (0.0, 0.0)
    for name, got, a, b in (("q", q, q64, q32), ("t", t, t64, t32), ("row", row, row64, row32)):
        v, r_max, r_rms = _violations(name, got, a, b)
        bad += v
        worst = (max(worst[0], r_max), max(worst[1], r_rms))
    # the row against the q, t this launch returned
    assert torch.equal(bits(row[:, :3]), bits(t))
    v, _, _ = _violations("row[3:]|q", row[:, 3:], PC.normalise_q(q, torch.float64), PC.normalise_q(q, torch.float32))
    bad += v
    print("  worst ratio kernel / E32: max %.2f rms %.2f (bound 4)" % worst)
    assert not bad, "; ".join(bad)
    others = [l for l in range(4) if l != case.level]
    assert (bits(pose[:, others]) == bits(torch.tensor(SENTINEL))).all(), "a row of another level was written"
    if nxt is not None:
        pose_w = torch.full((PC.B_HEAD, 4, 7), SENTINEL, device=cuda)
        q_w, t_w, warped = head(emb, logits, pose_w, case.level, q_prev, t_prev, warp_next=nxt)
        assert torch.equal(bits(q_w), bits(q)) and torch.equal(bits(t_w), bits(t)) and torch.equal(bits(pose_w), bits(pose))
        assert torch.equal(bits(warped), bits(fused.quat_warp_pm(nxt, q_w, t_w)))
        assert torch.equal(warped.cpu(), torch.from_numpy(PC.warp_expr(nxt, q_w, t_w, True)))


@pytest.mark.parametrize("N,spread,seed", PC.POOL_CASES, ids=["n%d_%s" % c[:2] for c in PC.POOL_CASES])
def test_masked_pool_against_float64(cuda, N, spread, seed):
    """``fused.masked_pool`` (masked_pool_kernel: 16 point slices per channel) on 8 x 64 pooled features against the
    float64 model by the same criterion; finite under logits over +-80 and +-100."""
    emb, logits = PC.pool_inputs(N, spread, seed)
    ex64, ex32 = PC.pool_reference(N, spread, seed)
    out = fused.masked_pool(emb.to(cuda), logits.to(cuda))
    print("\nN=%d %s:" % (N, spread))
    bad, _, _ = _violations("pooled", out, ex64, ex32)
    assert torch.isfinite(out).all()
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("case", PC.WARP_CASES, ids=[c.name for c in PC.WARP_CASES])
def test_quat_warp_is_the_reference_expression(cuda, case):
    """Both kernels equal ``warp_expr`` in float32 element for element (q = 0 included: the result is t, the sign of a
    zero is not asserted), and agree with each other bit for bit on the transposed cloud."""
    xyz, q, t = PC.warp_inputs(case)
    want = torch.from_numpy(PC.warp_expr(xyz, q, t, True))
    out_pm = fused.quat_warp_pm(xyz.to(cuda), q.to(cuda), t.to(cuda))
    out_cm = _ext.quat_warp(pm(xyz).to(cuda), q.to(cuda), t.to(cuda))
    assert torch.equal(out_pm.cpu(), want)
    assert torch.equal(out_cm.cpu(), torch.from_numpy(PC.warp_expr(pm(xyz), q, t, False)))
    assert torch.equal(bits(pm(out_cm)), bits(out_pm))
    if case.q_form == "zero":
        assert (out_pm.cpu() == t[:, None, :]).all()


def test_warp_batch_limit_is_reported(cuda):
    """B = 65536 clouds exceed the grid's y limit: both wrappers raise before any launch; B = 65535 is computed."""
    g = torch.Generator().manual_seed(77)
    B = 65536
    xyz = (torch.rand(B, 1, 3, generator=g) * 2 - 1) * 30
    q = torch.nn.functional.normalize(torch.randn(B, 4, generator=g), dim=1)
    t = torch.randn(B, 3, generator=g)
    dx, dq, dt = xyz.to(cuda), q.to(cuda), t.to(cuda)
    with pytest.raises(RuntimeError, match="grid limit"):
        fused.quat_warp_pm(dx, dq, dt)
    with pytest.raises(RuntimeError, match="grid limit"):
        _ext.quat_warp(pm(dx), dq, dt)
    want = torch.from_numpy(PC.warp_expr(xyz[:-1], q[:-1], t[:-1], True))
    assert torch.equal(fused.quat_warp_pm(dx[:-1].contiguous(), dq[:-1].contiguous(), dt[:-1].contiguous()).cpu(), want)
    assert torch.equal(_ext.quat_warp(pm(dx[:-1]), dq[:-1].contiguous(), dt[:-1].contiguous()).cpu(), pm(want))
