"""Every stack-kernel instantiation the three wrappers' dispatch can select (csrc/fused_layers.hip, fused_hoisted.hip,
fused_sa.hip), each at the smallest ragged shape that selects it and in every weight format it exists in, against the
float64 host model of tests/stack_reference.py.

One table (``stack_cases.CASES``), one comparison (``check``).  A row names the kernel instantiation(s) it is meant to
reach; the test runs the row inside ``_lib.launches()`` and first asserts that the kernels the library's launch layer
recorded, in launch order, are exactly those -- the launch itself, not a prediction of it (tests/test_stack_plan_cpu.py
asserts the same of every row as a dry run on the CPU) -- and then asserts the criterion of its format (``pytest -s``
prints every figure):

* fp32-accurate variants (fp32 and bf16x3 tiles) against ("exact", float64): max and RMS error each within 4 x E32, the
  CPU's own fp32 error on the same inputs, and the suite's 1e-5 mixed bound.  The margin of 4 covers the other summation
  order; a split layer that drops one of its six products sits at 9 x (max) / 14 x (RMS), test_stack_reference_cpu.py.
* bf16 tiles: R = RMS(kernel - ("bf16", float64)) <= Ebf / 8 with Ebf = RMS(("bf16", float64) - exact), max |kernel -
  exact| <= 2 x max |model - exact|, all finite.  A kernel that truncates sits at R / Ebf = 2.3 (same file).  R / R_ref
  (R_ref: the model in fp32 against the model in float64) is printed, not asserted.  test_stack_reference_cpu.py shows
  on the CPU that every bf16 row's inputs leave the bound alone (4 R_ref <= Ebf / 8).
  A stack without any rounding point (psa_1: no even layer, no hoisted rows) computes in fp32 in every format: its
  model has Ebf = 0 and the fp32 criterion applies.

The switches the library reads once per process (PWCLO_FL_WIDE, PWCLO_COARSE_W4, PWCLO_LANE6, PWCLO_LANE_UP) are set
for ONE fresh child process that runs ``CHILD_CASES`` through the same comparison and prints one JSON line per case.
"""
import json
import os
import subprocess
import sys
import time

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":                       # the child process: no conftest to set the paths up
    sys.path[:0] = [os.path.dirname(HERE), HERE]

import stack_reference as SR                                                     # noqa: E402
from pwclonet_pylidarslam_amd import fused                                       # noqa: E402
from stack_cases import B16, CASES, CHILD_CASES, CHILD_ENV, bf16_row_figures, launched, reference    # noqa: E402

pytestmark = pytest.mark.gpu

CHILD_TIME_LIMIT = 13       # seconds: 3 x the child's largest measured wall time, 4.2 s (profiles/stack_variants/README.md)


def check(case, dev):
    """Run one case -> (figures per output, violations).  Asserts the variant selection itself."""
    outs, records = launched(case, dev)
    names = [r[1] for r in records]
    assert names == case.want, "the library launched %s, the row is meant for %s" % (names, case.want)
    outs = [None if o is None else o.detach().cpu() for o in outs]
    ex = reference(case, SR.EXACT, torch.float64)
    use_bf16 = case.fmt == B16 and any(
        (a - b).abs().max().item() > 0 for a, b in zip(reference(case, SR.BF16, torch.float64), ex))
    figs, bad = [], []
    if use_bf16:
        for f in bf16_row_figures(case, outs):
            figs.append(dict(f, criterion="bf16", r_over_r_ref=f["r"] / f["r_ref"] if f["r_ref"] else float("inf")))
            bad += SR.bf16_violations(f)
    else:
        e32 = reference(case, SR.EXACT, torch.float32)
        for j, o in enumerate(outs):
            if o is not None:
                f = SR.fp32_figures(o, ex[j], e32[j])
                figs.append(dict(f, criterion="fp32"))
                bad += SR.fp32_violations(f)
    return figs, bad


def show(case, figs):
    for f in figs:
        if f["criterion"] == "fp32":
            print("\n%s [%s] %s: scale %.3g  E32 max %.3e rms %.3e | kernel max %.3e (%.2f x) rms %.3e (%.2f x)" % (
                case.want, case.fmt, case.shape if len(str(case.shape)) < 80 else "", f["scale"], f["e32_max"],
                f["e32_rms"], f["k_max"], f["k_max"] / f["e32_max"], f["k_rms"], f["k_rms"] / f["e32_rms"]))
        else:
            print("\n%s [%s]: scale %.3g  Ebf %.3e  R %.3e (Ebf / R = %.0f)  R_ref %.3e  R / R_ref %.2f | max: kernel "
                  "%.3e model %.3e" % (case.want, case.fmt, f["scale"], f["ebf"], f["r"], f["ebf"] / max(f["r"], 1e-300),
                                       f["r_ref"], f["r_over_r_ref"], f["k_max"], f["model_max"]))


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_stack_variant_against_float64(cuda, monkeypatch, case):
    for k, v in case.setenv.items():
        monkeypatch.setenv(k, v)
    with fused.packing_dtype(case.fmt):
        figs, bad = check(case, cuda)
    show(case, figs)
    assert not bad, "%s [%s]: %s" % (case.want, case.fmt, "; ".join(bad))


def test_switched_off_geometry_in_a_child_process(cuda):
    """PWCLO_FL_WIDE=0 PWCLO_COARSE_W4=0 PWCLO_LANE6=0 PWCLO_LANE_UP=0 are read once per process: one fresh child (two
    processes on the GPU) runs CHILD_CASES through ``check`` and prints a JSON line per case; the fp32 criterion is
    asserted here.  A non-zero exit or the time limit fails the test with the child's stderr; nothing is retried."""
    t0 = time.time()
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, **CHILD_ENV),
                           capture_output=True, text=True, timeout=CHILD_TIME_LIMIT)
    print("\nchild: %.1f s" % (time.time() - t0))
    assert child.returncode == 0, "child exited with %d:\n%s" % (child.returncode, child.stderr[-4000:])
    rows = [json.loads(line) for line in child.stdout.splitlines() if line.startswith("{")]
    assert [r["want"] for r in rows] == [c.want for c in CHILD_CASES]
    for r in rows:
        print(r)
        for f in r["figures"]:
            assert not SR.fp32_violations(f), (r["want"], SR.fp32_violations(f))


def _child():
    dev = torch.device("cuda:0")
    for case in CHILD_CASES:
        figs, _ = check(case, dev)              # a shape that selects another variant ends the child: AssertionError
        print(json.dumps(dict(want=case.want, figures=figs)), flush=True)


if __name__ == "__main__":
    assert sys.argv[1:] == ["--child"]
    _child()
