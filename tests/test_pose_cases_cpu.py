"""tests/pose_cases.py on the CPU: the cases of tests/test_gpu_pose_path.py discriminate.

* A correct float32 pose head that sums the pooling in another order (the kernel's 64 slots) passes the fp32 criterion of
  tests/stack_reference.py on every case, with both ratios to E32 at most 2: half the bound of 4.
* ``warp_expr`` in float32 is the oracle's ``warp`` bit for bit and within the 1e-5 mixed bound of its float64 evaluation.
* Every mutant of ``pose_cases.MUTANTS`` -- a host model wrong in one way a kernel could be -- is caught by a case.

Run with ``-s`` for the figures."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_cases as PC                                                          # noqa: E402
import stack_reference as SR                                                     # noqa: E402
from oracle import model as M                                                    # noqa: E402

pm = lambda t: t.permute(0, 2, 1).contiguous()      # (B,C,N) <-> (B,N,C)


def _ratio(a, b):
    return a / b if b > 0 else (0.0 if a == 0 else float("inf"))


def _judge(case, outputs):
    """``outputs`` = (pooled, q, t, row) of some float32 implementation -> (violations, worst max ratio, worst RMS ratio)."""
    ex64, ex32 = PC.head_reference(case.name)
    bad, r_max, r_rms = [], 0.0, 0.0
    for name, got, a, b in zip(PC.HEAD_OUTPUTS, outputs, ex64, ex32):
        f = SR.fp32_figures(got, a, b)
        bad += ["%s: %s" % (name, v) for v in SR.fp32_violations(f)]
        r_max, r_rms = max(r_max, _ratio(f["k_max"], f["e32_max"])), max(r_rms, _ratio(f["k_rms"], f["e32_rms"]))
    return bad, r_max, r_rms


def _run(case, **kw):
    x = PC.head_inputs(case)
    return PC.head_model(x["emb"], x["logits"], PC.head_weights(), x["q_prev"], x["t_prev"], torch.float32, **kw)


def test_head_model_in_fp32_is_the_oracles_pose_head():
    """The model in float32 against oracle/model.py's own functions (which the whole-network goldens pin to the
    reference): pose_calculator bit for bit, the composition and the row within the 1e-5 mixed bound (the oracle sums
    |q|^2 with torch.sum, the model left to right)."""
    case = PC.HEAD_BY_NAME["n1000_prev_w2049"]
    x = PC.head_inputs(case)
    names = ("conv1d_q_t", "conv1d_q", "conv1d_t")
    sd = {"%s.%s.conv.%s" % (PC.PREFIX, names[i // 2], ("weight", "bias")[i % 2]): w for i, w in enumerate(PC.head_weights())}
    emb, logits = pm(x["emb"]), pm(x["logits"])
    qd, td = M.pose_calculator(sd, PC.PREFIX, emb, torch.softmax(logits, dim=2))
    pooled, q4, t4, row4 = PC.head_model(x["emb"], x["logits"], PC.head_weights(), None, None, torch.float32)
    assert torch.equal(pooled, torch.sum(emb * torch.softmax(logits, dim=2), dim=2))
    assert torch.equal(q4, qd.squeeze(2)) and torch.equal(t4, td.squeeze(2))
    assert SR.close_1e5(row4, torch.cat((td.squeeze(2), M._normalise_q(qd.squeeze(2))), dim=1)) == 0
    _, q, t, row = PC.head_reference(case.name)[1]
    ref_q = M._hamilton(qd, x["q_prev"].reshape(-1, 4, 1)).squeeze(2)
    ref_t = M.warp(x["t_prev"].reshape(-1, 3, 1), qd, td).squeeze(2)
    assert torch.equal(q, ref_q)
    assert SR.close_1e5(t, ref_t) == 0
    assert SR.close_1e5(row, torch.cat((ref_t, M._normalise_q(ref_q)), dim=1)) == 0


def test_case_table_reaches_every_form():
    """The table against pose_head_kernel's branches: both q_prev forms with and without the warp, warps of more than one
    trip in both forms, N below, at and above the slot count and the unroll, every level row, every logit spread."""
    C = PC.HEAD_CASES
    assert all(len(c.why) > 10 for c in C) and len({c.name for c in C}) == len(C) <= 22
    assert {c.N for c in C} >= {1, 3, 63, 64, 65, 255, 256, 257, 1000}
    assert {(c.N, c.spread) for c in C} >= {(256, "u80"), (65, "u80")}
    assert {c.prev for c in C} == {None, 1.0, 1.7, 0.3}
    assert {c.level for c in C} == {0, 1, 2, 3}
    assert {c.warp_n for c in C} == {0, 1, 777, 1023, 1024, 1025, 2049}
    forms = {(c.prev is not None, c.warp_n) for c in C}
    assert forms >= {(p, w) for p in (False, True) for w in (0, 1025, 2049)}
    W = PC.WARP_CASES
    assert {(c.n, c.q_form) for c in W} == {(n, f) for n in (1, 255, 256, 257, 2049) for f in PC.Q_FORMS}
    assert {(c.n, c.B) for c in W} == {(n, b) for n in (1, 255, 256, 257, 2049) for b in (1, 3)}
    assert {(c.q_form, c.B) for c in W} == {(f, b) for f in PC.Q_FORMS for b in (1, 3)}


def test_correct_fp32_head_in_the_kernels_order_passes_with_margin():
    """``head_model(float32, order="slots")`` against the float64 model, E32 from the plain float32 evaluation: no
    violation, and both ratios at most 2 on the committed seeds, so the bound of 4 leaves a correct implementation in
    another summation order alone.  (A case that misses this gets another seed, never another criterion.)"""
    print()
    failures = []
    for case in PC.HEAD_CASES:
        bad, r_max, r_rms = _judge(case, _run(case, order="slots"))
        print("  %-22s slots model / E32: max %.2f  rms %.2f" % (case.name, r_max, r_rms))
        if bad or r_max > 2 or r_rms > 2:
            failures.append("%s: max %.2f rms %.2f %s" % (case.name, r_max, r_rms, "; ".join(bad)))
    assert not failures, "\n".join(failures)


def test_pool_cases_pass_with_margin():
    """The same for the inputs of test_masked_pool_against_float64."""
    print()
    for N, spread, seed in PC.POOL_CASES:
        emb, logits = PC.pool_inputs(N, spread, seed)
        ex64, ex32 = PC.pool_reference(N, spread, seed)
        f = SR.fp32_figures(PC.pool_model(emb, logits, torch.float32, order="slots"), ex64, ex32)
        r_max, r_rms = _ratio(f["k_max"], f["e32_max"]), _ratio(f["k_rms"], f["e32_rms"])
        print("  N=%-4d %-6s slots model / E32: max %.2f  rms %.2f" % (N, spread, r_max, r_rms))
        assert not SR.fp32_violations(f) and r_max <= 2 and r_rms <= 2, (N, spread, f)


@pytest.mark.parametrize("case", PC.WARP_CASES, ids=[c.name for c in PC.WARP_CASES])
def test_warp_expr_is_the_oracles_warp(case):
    """``warp_expr`` in float32 equals ``oracle.model.warp`` bit for bit for unit and scaled q, in both layouts (for
    these inputs torch.sum's order over the four q_i^2 gives the same |q|^2 as the left-to-right sum, so no case is
    excluded), and lies within the 1e-5 mixed bound of its float64 evaluation; with |q|^2 below the epsilon and with
    q = 0 the float32 result is finite, and equal to t for q = 0."""
    xyz, q, t = PC.warp_inputs(case)
    got = PC.warp_expr(xyz, q, t, True)
    got_cm = PC.warp_expr(pm(xyz), q, t, False)
    assert got.dtype == np.float32 and np.array_equal(got.transpose(0, 2, 1), got_cm)
    assert np.isfinite(got).all()
    exact = PC.warp_expr(xyz, q, t, True, dtype=np.float64)
    if case.q_form in ("unit", "x1.7"):
        ref = M.warp(pm(xyz), q.reshape(-1, 4, 1), t.reshape(-1, 3, 1))
        assert np.array_equal(got_cm, ref.numpy())
        assert SR.close_1e5(torch.from_numpy(got), torch.from_numpy(exact)) == 0
    if case.q_form == "zero":
        assert (got == t.numpy()[:, None, :]).all()


def test_every_mutant_is_caught():
    """Head mutants: an fp32_violations entry or a non-finite value on at least one case.  Warp mutants: at least one
    output element with other bits."""
    print()
    caught = {m: [] for m in PC.MUTANTS}
    for m in PC.HEAD_MUTANTS:
        for case in PC.HEAD_CASES:
            if _judge(case, _run(case, order="slots", mutant=m))[0]:
                caught[m].append(case.name)
    for m in PC.WARP_MUTANTS:
        for case in PC.WARP_CASES:
            xyz, q, t = PC.warp_inputs(case)
            a, b = PC.warp_expr(xyz, q, t, True), PC.warp_expr(xyz, q, t, True, mutant=m)
            if not np.array_equal(a.view(np.int32), b.view(np.int32)):
                caught[m].append(case.name)
    for m in PC.MUTANTS:
        print("  %-26s caught by %d: %s" % (m, len(caught[m]), ", ".join(caught[m]) or "NOTHING"))
    assert all(caught.values()), "uncaught: %s" % [m for m in PC.MUTANTS if not caught[m]]
