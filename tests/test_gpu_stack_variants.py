"""Every stack-kernel instantiation the three wrappers' dispatch can select (csrc/fused_layers.hip, fused_hoisted.hip,
fused_sa.hip), each at the smallest ragged shape that selects it and in every weight format it exists in, against the
float64 host model of tests/stack_reference.py.

One table (``CASES``), one comparison (``check``).  A row names the kernel instantiation(s) it is meant to reach; the
test first asserts that its shape, format and switches really select them -- through fused.py's name mirrors where one
exists, otherwise through the formulas below, restated from the wrapper lines named beside them -- and then asserts
the criterion of its format (``pytest -s`` prints every figure):

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

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":                       # the child process: no conftest to set the paths up
    sys.path[:0] = [os.path.dirname(HERE), HERE]

import stack_reference as SR                                                     # noqa: E402
from oracle import ops as O                                                      # noqa: E402
from oracle import params                                                        # noqa: E402
from pwclonet_pylidarslam_amd import fused                                       # noqa: E402
from pwclonet_pylidarslam_amd.pointnet2_ops.pointnet2_modules import (           # noqa: E402
    PointnetFPModulePWCLONet, PointnetSAModulePWCLONet)
from pwclonet_pylidarslam_amd.pwclonet import CostVolume, FlowPredictor          # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF3, B16 = "f32", "bf16x3", "bf16"
WFMT = {F32: fused.WFMT_F32, BF3: fused.WFMT_BF16X3, B16: fused.WFMT_BF16}
CHILD_ENV = {"PWCLO_FL_WIDE": "0", "PWCLO_COARSE_W4": "0", "PWCLO_LANE6": "0", "PWCLO_LANE_UP": "0"}
CHILD_TIME_LIMIT = 13       # seconds: 3 x the child's largest measured wall time, 4.2 s (profiles/stack_variants/README.md)


def filled(module, prefix):
    sd = module.state_dict()
    for k, v in sd.items():
        v.copy_(torch.from_numpy(np.array(params.fill_value(prefix + "." + k, v.shape))).reshape(v.shape).to(v.dtype))
    return module.eval()


def cloud(seed, b, n, scale=10.0):
    return (torch.rand(b, n, 3, generator=torch.Generator().manual_seed(seed)) * 2 - 1) * scale


def randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def env(name, dflt):
    return int(os.environ.get(name, dflt))


# ---- the dispatch, restated ------------------------------------------------------------------------------------------

def stack_tiles(b, s, kp, p):
    """csrc/launch.hpp stack_tiles: b clouds of s queries with kp pixel slots, tiles of p 16-pixel blocks."""
    return b * ((s * kp + 16 * p - 1) // (16 * p))


def coarse(tiles):
    """csrc/launch.hpp coarse_w4() / coarse_tiles(): a launch this small takes 4-wave workgroups."""
    return env("PWCLO_COARSE_W4", 1) != 0 and tiles <= env("PWCLO_COARSE_W4_TILES", 2047)


def pointwise_name(chans, w1, w2, b, s, tail=0):
    """csrc/fused_layers.hip launch_pointwise: 4 waves when coarse(b * ceil(s / 16)), else 16; the <.., 2, 8> form
    without PWCLO_FL_WIDE (the stack + tail form is always wide)."""
    nb = [c // 16 for c in chans] + [0] * (3 - len(chans))
    head = "pointwise_kernel<%d, %d, %d, %d, %d, " % (*nb, w1 // 16, w2 // 16)
    wide = tail > 0 or env("PWCLO_FL_WIDE", 1) != 0
    if wide:
        return head + "1, %d, %d>" % (4 if coarse(stack_tiles(b, s, 1, 1)) else 16, tail // 16)
    return head + "2, 8, 0>"


def sa_h_name(widths, k, lvl0, kmajor, b, s, wfmt):
    """csrc/fused_hoisted.hip sa_fused_h_kernel_wrapper: SAH_CASE by widths; flow-feature encoding (128, 64, 64) on 4
    waves when coarse(b * s)."""
    kp = 32 if k > 16 else 16
    if kmajor:
        return "sa_h_kernel<1, 1, 1, 32, 2, 8, true, 0, true>"
    p, w = {(16, 16, 16): (2, 8), (16, 16, 32): (2, 8), (32, 32, 64): (1, 16), (64, 64, 128): (1, 16),
            (128, 64, 64): (1, 4 if coarse(stack_tiles(b, s, 16, 1)) else 16)}[tuple(widths)]
    return "sa_h_kernel<%d, %d, %d, %d, %d, %d, %s, %d>" % (*[c // 16 for c in widths], kp, p, w,
                                                           "true" if lvl0 else "false", wfmt)


def unhoisted_names(kq, b, s):
    """csrc/fused_layers.hip upconv_fused / cv_fused_a1 / cv_fused_b wrappers: <.., 1, 16> with PWCLO_FL_WIDE, else
    <.., 2, 8> (cv_a1 with 32 slots: always <.., 2, 8>)."""
    wide = env("PWCLO_FL_WIDE", 1) != 0
    kp = fused.cv_pix_slots(kq)
    return dict(up="upconv_kernel<8, %s>" % ("1, 16" if wide else "2, 8"),
                a1="cv_a1_kernel<%%d, %d, %s>" % (kp, "1, 16" if wide and kp <= 16 else "2, 8"),
                b="cv_b_kernel<%%d, 4, %s>" % ("1, 16" if wide else "2, 8"))


# ---- cases -----------------------------------------------------------------------------------------------------------

class Case:
    """One table row.  ``want``: the kernel instantiation(s) the row is meant to reach; ``fmt``: weight format;
    ``setenv``: variables fused.py reads per call or at pack time (monkeypatch reaches those)."""
    kind = ""

    def __init__(self, want, fmt=F32, setenv=None, **shape):
        self.want = [want] if isinstance(want, str) else list(want)
        self.fmt, self.setenv, self.shape = fmt, dict(setenv or {}), shape
        self.__dict__.update(shape)

    @property
    def id(self):
        return "-".join([self.want[0].replace(" ", ""), self.fmt, "x".join(
            str(v).replace(" ", "") for v in self.shape.values() if isinstance(v, (int, tuple)))] + list(self.setenv))

    def key(self):                                  # what the inputs and the exact references depend on
        return (self.kind, tuple(sorted((k, str(v)) for k, v in self.shape.items())))


class Pointwise(Case):
    kind = "pointwise"

    def inputs(self):
        chans, b, s = self.chans, self.b, self.s
        widths = self.shape.get("mlp", [128, 64])
        mod = filled(FlowPredictor(in_channel=sum(chans), mlp=list(widths)), "l4_flow_predictor")
        tail = None
        if self.shape.get("tail"):
            tail = (randn(19, 128, 64) * 0.2, randn(20, 128))
        return dict(mod=mod, srcs=[randn(30 + i, b, s, c) for i, c in enumerate(chans)], tail=tail)

    def model(self, i, **kw):
        out = SR.pointwise(i["mod"].mlp_convs, i["srcs"], tail=i["tail"], **kw)
        return out if isinstance(out, tuple) else (out,)

    def run(self, i, dev):
        pw = fused.FusedPointwise(i["mod"].to(dev).mlp_convs, list(self.chans))
        srcs = [t.to(dev) for t in i["srcs"]]
        name = pointwise_name(self.chans, pw.w1, pw.w2, self.b, self.s, 128 if i["tail"] else 0)
        if i["tail"] is None:
            return (pw(*srcs),), [name]
        job = fused.LinearJob(i["tail"][0].to(dev), i["tail"][1].to(dev))
        assert pw.tail_supported(job)
        return pw.with_tail(job, *srcs), [name]


class SetAbstraction(Case):
    kind = "sa"

    def inputs(self):
        b, n, s, k, c = self.b, self.n, self.s, self.k, self.mlp[0]
        mod = filled(PointnetSAModulePWCLONet(mlp=list(self.mlp), npoint=s, nsample=k), self.name)
        xyz = cloud(1, b, n)
        new_xyz = xyz[:, :s].contiguous() + 0.01
        return dict(mod=mod, xyz=xyz, new_xyz=new_xyz, feat=randn(2, b, n, c) if c else None,
                    idx=O.knn_point_with_dist(k, xyz, new_xyz)[1])

    def model(self, i, **kw):
        return (SR.set_abstraction(i["mod"], i["xyz"], i["new_xyz"], i["feat"], i["idx"], **kw),)

    def run(self, i, dev):
        fsa = fused.FusedSAHoisted(i["mod"].to(dev))
        assert fsa.wfmt == WFMT[self.fmt]
        pre = fused.run_linear_jobs(fsa.jobs(i["feat"].to(dev)))[0] if i["feat"] is not None else None
        assert pre is None or (pre.dtype == torch.bfloat16) == (self.fmt == B16)
        out = fsa(i["xyz"].to(dev), i["new_xyz"].to(dev), pre, i["idx"].to(dev))
        return (out,), [sa_h_name(fsa.widths, self.k, pre is None, fsa.kmajor, self.b, self.s, fsa.wfmt)]


def _upconv_module(name, c2):
    return filled(PointnetFPModulePWCLONet(nsample=8, mlp=[64, 128, 64], post_mlp=[64 + c2, 64], radius=0.2, knn=True,
                                           use_xyz=True, bn=True), name)


class Upconv(Case):
    """Hoisted set-upconv + its post-MLP as separate launches; ``hoist=False``: the un-hoisted kernel."""
    kind = "upconv"

    def inputs(self):
        b, n2, n1, k, c2 = self.b, self.s, self.n, self.k, self.c2
        xyz2, xyz1 = cloud(3, b, n2), cloud(4, b, n1)
        return dict(mod=_upconv_module("pose_warp_refinement_2.setupconv_features", c2), xyz2=xyz2, xyz1=xyz1,
                    f2=randn(5, b, n2, c2), f1=randn(6, b, n1, 64), idx=O.knn_point_with_dist(k, xyz1, xyz2)[1])

    def model(self, i, **kw):
        return (SR.set_upconv(i["mod"], i["xyz2"], i["xyz1"], i["f2"], i["f1"], i["idx"], **kw),)

    def run(self, i, dev):
        g = {k_: v.to(dev) for k_, v in i.items() if k_ != "mod"}
        post = pointwise_name((64, self.c2), 64, 0, self.b, self.s)
        if not self.shape.get("hoist", True):
            up = fused.FusedUpconv(i["mod"].to(dev))
            return (up(g["xyz2"], g["xyz1"], g["f2"], g["f1"], g["idx"]),), [unhoisted_names(6, self.b, self.s)["up"], post]
        up = fused.FusedUpconvHoisted(i["mod"].to(dev))
        assert up.wfmt == WFMT[self.fmt]
        (pre,) = fused.run_linear_jobs(up.jobs(g["f1"]))
        out = up(g["xyz2"], g["xyz1"], g["f2"], pre, g["idx"])
        return (out,), [fused._upconv_h_kernel_name(self.b, self.s, up.wfmt), post]


class UpconvPost(Case):
    """Both set-upconvs of a level and their post-MLPs as one launch."""
    kind = "upconv_post"
    NAMES = ["pose_warp_refinement_2.setupconv_features", "pose_warp_refinement_2.setupconv_mask"]

    def inputs(self):
        b, n2, n1, k, c2 = self.b, self.s, self.n, self.k, self.c2
        xyz2, xyz1 = cloud(3, b, n2), cloud(4, b, n1)
        return dict(mods=[_upconv_module(nm, c2) for nm in self.NAMES[:self.njobs]], xyz2=xyz2, xyz1=xyz1,
                    f2=randn(5, b, n2, c2), f1s=[randn(6 + j, b, n1, 64) for j in range(self.njobs)],
                    idx=O.knn_point_with_dist(k, xyz1, xyz2)[1])

    def model(self, i, **kw):
        return tuple(SR.set_upconv(m, i["xyz2"], i["xyz1"], i["f2"], f1, i["idx"], **kw)
                     for m, f1 in zip(i["mods"], i["f1s"]))

    def run(self, i, dev):
        ups = [fused.FusedUpconvHoisted(m.to(dev)) for m in i["mods"]]
        pres = fused.run_linear_jobs([u.jobs(f1.to(dev))[0] for u, f1 in zip(ups, i["f1s"])])
        outs = fused.run_upconv_post(ups, i["xyz2"].to(dev), i["xyz1"].to(dev), i["f2"].to(dev), pres, i["idx"].to(dev))
        return tuple(outs), [fused._upconv_post_kernel_name(self.njobs, self.b, self.s, self.c2)]


class CostVol(Case):
    """The whole cost volume (first aggregate a1 + a2, then b); compared on ``first`` and on the result.
    ``hoist=False``: the un-hoisted kernels."""
    kind = "cv"

    def inputs(self):
        b, s, n, c, kq = self.b, self.s, self.n, self.c, self.kq
        mod = filled(CostVolume(nsample=4, nsample_q=kq, in_channel1=c, in_channel2=c, mlp1=[128, 64, 64],
                                mlp2=[128, 64]), "cost_volume")
        x1, x2 = cloud(7, b, s), cloud(8, b, n)
        return dict(mod=mod, x1=x1, x2=x2, p1=randn(9, b, s, c), p2=randn(10, b, n, c),
                    idx_q=O.knn_point_with_dist(kq, x2, x1)[1], idx=O.knn_point_with_dist(4, x1, x1)[1])

    def model(self, i, **kw):
        return SR.cost_volume(i["mod"], i["x1"], i["p1"], i["x2"], i["p2"], i["idx_q"], i["idx"],
                              hoisted=self.shape.get("hoist", True), **kw)

    def run(self, i, dev):
        g = {k_: v.to(dev) for k_, v in i.items() if k_ != "mod"}
        b, s, kq = self.b, self.s, self.kq
        kp = fused.cv_pix_slots(kq)
        if not self.shape.get("hoist", True):
            cv = fused.FusedCostVolume(i["mod"].to(dev))
            assert cv.wfmt_a2 == fused.cv_stack_wfmt(kp, WFMT[self.fmt], hoisted=False)
            out = cv(g["x1"], g["p1"], g["x2"], g["p2"], idx_q=g["idx_q"], idx=g["idx"])
            un = unhoisted_names(kq, b, s)
            return (out, None), [un["a1"] % (self.c // 16), fused._a2_kernel_name(kp, b, s, cv.wfmt_a2),
                                 un["b"] % (self.c // 16)]
        cv = fused.FusedCostVolumeHoisted(i["mod"].to(dev))
        assert cv.wfmt == fused.cv_stack_wfmt(kp, WFMT[self.fmt]) and cv.job_u.out_bf16 == (cv.wfmt == fused.WFMT_BF16)
        u, v, u2 = fused.run_linear_jobs(cv.jobs(g["p1"], g["p2"]))
        seen, second = {}, cv._second

        def keep(xyz1, u2_, v2, first, idx):       # cv_b's inputs: the first aggregate is compared too
            seen["first"], seen["v2"] = first, v2
            return second(xyz1, u2_, v2, first, idx)
        cv._second = keep
        out = cv(g["x1"], g["x2"], u, v, u2, idx_q=g["idx_q"], idx=g["idx"])
        merged = (kp == 6 and cv.wfmt == fused.WFMT_F32 and b * ((s + 15) // 16) >= env("PWCLO_CV_MERGED_MIN", 512)
                  and env("PWCLO_LANE6", 1) != 0 and env("PWCLO_CV_MERGED", 1) != 0)     # fused.py FusedCostVolumeHoisted.__call__
        assert seen["v2"].dtype == (torch.bfloat16 if cv.wfmt == fused.WFMT_BF16 else torch.float32)
        if merged:
            names = [fused._a_lane6_kernel_name(b, s, env("PWCLO_CV_V2", 1) != 0)]
        else:
            names = [fused._a1_h_kernel_name(kp, cv.wfmt), fused._a2_kernel_name(kp, b, s, cv.wfmt_a2)]
        return (out, seen["first"]), names + [fused._b_h_kernel_name(b, s, cv.wfmt)]


class Linear(Case):
    """linear_jobs with bf16 rows: every job once with fp32 rows and once with bf16 rows in ONE launch."""
    kind = "linear"
    JOBS = [(16, 128, 500), (32, 64, 33), (64, 128, 2051), (64, 16, 7)]

    def inputs(self):
        return dict(jobs=[(randn(40 + j, co, ci) * 0.3, randn(50 + j, co), randn(60 + j, 1, n, ci))
                          for j, (ci, co, n) in enumerate(self.JOBS)])

    def model(self, i, **kw):
        return tuple(SR.linear_job(w, b, src, **kw) for w, b, src in i["jobs"])

    def run(self, i, dev):
        jobs = []
        for w, b, src in i["jobs"]:
            for h16 in (False, True):
                jobs.append((fused.LinearJob(w.to(dev), b.to(dev), out_bf16=h16), src.to(dev)))
        outs = fused.run_linear_jobs(jobs)
        for f32, b16 in zip(outs[0::2], outs[1::2]):
            assert b16.dtype == torch.bfloat16 and torch.equal(b16, f32.to(torch.bfloat16))      # bit for bit
        return tuple(outs[0::2]), ["linear_jobs_kernel"]


PW_SETS = [((64, 64), [64]), ((64, 32), [64]), ((64, 16), [64]), ((64, 64, 64), [128, 64]), ((32, 64, 64), [128, 64]),
           ((64, 64, 32), [128, 64]), ((16, 64, 64), [128, 64]), ((128, 64), [128, 64])]      # fused_layers.hip PW_CASE
SA_SETS = [("psa_1", [0, 8, 8, 16], 20, "sa_h_kernel<1, 1, 1, 32, 2, 8, true, 0, true>", {}),
           ("psa_1", [0, 8, 8, 16], 20, "sa_h_kernel<1, 1, 1, 32, 2, 8, true, %d>", {"PWCLO_SA_KMAJOR": "0"}),
           ("psa_2", [16, 16, 16, 32], 20, "sa_h_kernel<1, 1, 2, 32, 2, 8, false, %d>", {}),
           ("psa_3", [32, 32, 32, 64], 11, "sa_h_kernel<2, 2, 4, 16, 1, 16, false, %d>", {}),
           ("psa_4", [64, 64, 64, 128], 11, "sa_h_kernel<4, 4, 8, 16, 1, 16, false, %d>", {})]


def _table():
    t = []
    # pointwise_kernel: 2 x 203 rows = 26 tiles (4 waves); 2 x 16391 = 2050 tiles > 2047 (16 waves)
    for chans, mlp in PW_SETS:
        nb = [c // 16 for c in chans] + [0] * (3 - len(chans)) + [mlp[0] // 16, (mlp[1] if len(mlp) > 1 else 0) // 16]
        for s, w in ((203, 4), (16391, 16)):
            t.append(Pointwise("pointwise_kernel<%d, %d, %d, %d, %d, 1, %d, 0>" % (*nb, w), chans=chans, mlp=mlp, b=2, s=s))
    for chans in ((32, 64, 64), (64, 64, 32)):                                    # fused_layers.hip PWT_CASE
        for s, w in ((203, 4), (16391, 16)):
            t.append(Pointwise("pointwise_kernel<%d, %d, %d, 8, 4, 1, %d, 8>" % (*[c // 16 for c in chans], w),
                               chans=chans, b=2, s=s, tail=True))
    for fmt in (F32, BF3, B16):
        for name, mlp, k, want, setenv in SA_SETS:                               # K below its 32 / 16 slots
            t.append(SetAbstraction(want % WFMT[fmt] if "%d" in want else want, fmt, setenv, name=name, mlp=mlp, b=3,
                                    n=300, s=37, k=k))
        # flow-feature encoding: b * s = 192 tiles (4 waves), 3 x 683 = 2049 > 2047 (16 waves)
        for s, w in ((64, 4), (683, 16)):
            t.append(SetAbstraction("sa_h_kernel<8, 4, 4, 16, 1, %d, false, %d>" % (w, WFMT[fmt]), fmt,
                                    name="flow_feature_encoding", mlp=[64, 128, 64, 64], b=3, n=700, s=s, k=11))
        t.append(Upconv(["upconv_h_kernel<8, 1, 16, %d>" % WFMT[fmt], "pointwise_kernel<4, 2, 0, 4, 0, 1, 4, 0>"], fmt,
                        c2=32, b=2, s=333, n=90, k=5))
    # b * ceil(s / 16) = 2 x 1026 = 2052 > 2048 (fused_hoisted.hip upconv_fused_h_kernel_wrapper)
    t.append(Upconv(["upconv_lane_kernel<16>", "pointwise_kernel<4, 1, 0, 4, 0, 1, 16, 0>"], c2=16, b=2, s=16403, n=700, k=8))
    # fused_hoisted.hip launch_upconv_post: njobs * b * ceil(s / 16) = 20 (4 waves), 2052 in [2048, 4096) (8), 4104 (16)
    for c2 in (16, 32, 64):
        for s, w in ((77, 4), (8197, 8), (16403, 16)):
            t.append(UpconvPost("upconv_lane_post_kernel<%d, %d>" % (c2 // 16, w), c2=c2, njobs=2, b=2, s=s, n=300, k=8))
    for fmt in (F32, BF3, B16):
        f = WFMT[fmt]
        # 6 slots, 2 x 301 queries: t6 = 76 (dense-6 on 4 waves), 152 cv_b tiles (4 waves)
        t.append(CostVol(["cv_a1_h_kernel<6, 1, 16, %d>" % f, "cv_a2_dense6_kernel<4, %d>" % f,
                          "cv_b_h_kernel<4, 1, 4, %d>" % f], fmt, c=16, kq=6, b=2, s=301, n=280))
        # 32 slots with K = 20 < 32
        t.append(CostVol(["cv_a1_h_kernel<32, 1, 16, %d>" % f, "cv_a2_kernel<32, 2, 8, %d>" % f,
                          "cv_b_h_kernel<4, 1, 4, %d>" % f], fmt, c=64, kq=20, b=2, s=70, n=90))
    # t6 = 2 x 1025 = 2050 > 2048 (fused_layers.hip cv_fused_a2_kernel_wrapper); cv_b: 2 x 2050 tiles > 2047 (16 waves)
    for fmt in (BF3, B16):
        f = WFMT[fmt]
        t.append(CostVol(["cv_a1_h_kernel<6, 1, 16, %d>" % f, "cv_a2_dense6_kernel<8, %d>" % f,
                          "cv_b_h_kernel<4, 1, 16, %d>" % f], fmt, c=16, kq=6, b=2, s=8197, n=8190))
    t.append(CostVol(["cv_a1_h_kernel<8, 1, 16, 0>", "cv_a2_kernel<8, 1, 16, 0>", "cv_b_h_kernel<4, 1, 4, 0>"],
                     c=32, kq=5, b=2, s=37, n=64))                               # 8 slots, K = 5
    t.append(CostVol(["cv_a1_h_kernel<16, 1, 16, 0>", "cv_a2_kernel<16, 1, 16, 0>", "cv_b_h_kernel<4, 1, 4, 0>"],
                     c=64, kq=11, b=2, s=37, n=64))                              # 16 slots, K = 11
    t.append(CostVol(["cv_a1_h_kernel<16, 1, 16, 0>", "cv_a2_kernel<16, 1, 16, 0>", "cv_b_h_kernel<4, 1, 4, 0>"],
                     B16, c=64, kq=11, b=2, s=37, n=64))                         # bf16 asked for: 16 slots run fp32
    # t16 = 2 x 513 = 1026 > 1024: the in-lane a2 (separate kernels) and the one-kernel first aggregate on 8 waves
    t.append(CostVol(["cv_a1_h_kernel<6, 1, 16, 0>", "cv_a2_lane6_kernel<8>", "cv_b_h_kernel<4, 1, 16, 0>"],
                     setenv={"PWCLO_CV_MERGED": "0"}, c=16, kq=6, b=2, s=8197, n=8190))
    t.append(CostVol(["cv_a_lane6_kernel<8, true>", "cv_b_h_kernel<4, 1, 16, 0>"], c=16, kq=6, b=2, s=8197, n=8190))
    t.append(CostVol(["cv_a_lane6_kernel<8, false>", "cv_b_h_kernel<4, 1, 16, 0>"], setenv={"PWCLO_CV_V2": "0"},
                     c=16, kq=6, b=2, s=8197, n=8190))
    # t16 = 2 x 257 = 514 in [512, 1024]: one-kernel first aggregate on 4 waves; cv_b: 2 x 1025 = 2050 tiles (16 waves)
    t.append(CostVol(["cv_a_lane6_kernel<4, true>", "cv_b_h_kernel<4, 1, 16, 0>"], c=32, kq=6, b=2, s=4099, n=4000))
    # un-hoisted cost volume with bf16x3: only cv_a2 takes the split format (6 / 32 slots)
    t.append(CostVol(["cv_a1_kernel<1, 6, 1, 16>", "cv_a2_dense6_kernel<4, 1>", "cv_b_kernel<1, 4, 1, 16>"], BF3,
                     hoist=False, c=16, kq=6, b=2, s=301, n=280))
    t.append(CostVol(["cv_a1_kernel<4, 32, 2, 8>", "cv_a2_kernel<32, 2, 8, 1>", "cv_b_kernel<4, 4, 1, 16>"], BF3,
                     hoist=False, c=64, kq=20, b=2, s=70, n=90))
    t.append(Linear("linear_jobs_kernel"))
    return t


CASES = _table()

# PWCLO_FL_WIDE=0 PWCLO_COARSE_W4=0 PWCLO_LANE6=0 PWCLO_LANE_UP=0, fp32 tiles: the kernels those switches "restore"
CHILD_CASES = [
    Pointwise("pointwise_kernel<4, 4, 4, 8, 4, 2, 8, 0>", chans=(64, 64, 64), mlp=[128, 64], b=2, s=203),
    Pointwise("pointwise_kernel<2, 4, 4, 8, 4, 1, 16, 8>", chans=(32, 64, 64), b=2, s=203, tail=True),   # small, now 16 waves
    Upconv(["upconv_kernel<8, 2, 8>", "pointwise_kernel<4, 2, 0, 4, 0, 2, 8, 0>"], hoist=False, c2=32, b=2, s=333, n=90, k=5),
    CostVol(["cv_a1_kernel<2, 8, 2, 8>", "cv_a2_kernel<8, 2, 8, 0>", "cv_b_kernel<2, 4, 2, 8>"], hoist=False,
            c=32, kq=5, b=2, s=37, n=64),
    CostVol(["cv_a1_h_kernel<16, 1, 16, 0>", "cv_a2_kernel<16, 2, 8, 0>", "cv_b_h_kernel<4, 1, 16, 0>"],
            c=64, kq=11, b=2, s=37, n=64),                                       # small, now the 16-wave cv_b_h
    CostVol(["cv_a1_h_kernel<6, 1, 16, 0>", "cv_a2_dense6_kernel<8, 0>", "cv_b_h_kernel<4, 1, 16, 0>"],
            c=16, kq=6, b=2, s=8197, n=8190),                                    # t6 = 2050 > 2048
    Upconv(["upconv_h_kernel<8, 1, 16, 0>", "pointwise_kernel<4, 1, 0, 4, 0, 2, 8, 0>"], c2=16, b=2, s=16403, n=700, k=8),
    SetAbstraction("sa_h_kernel<8, 4, 4, 16, 1, 16, false, 0>", name="flow_feature_encoding", mlp=[64, 128, 64, 64],
                   b=3, n=700, s=64, k=11),                                      # small, now 16 waves
]


# ---- the comparison --------------------------------------------------------------------------------------------------

_INPUTS, _REFS = {}, {}


def inputs_of(case):
    if case.key() not in _INPUTS:
        _INPUTS[case.key()] = case.inputs()
    return _INPUTS[case.key()]


def reference(case, rounding, dtype):
    """Computed once per (inputs, rounding, type) and shared by the rows that use the same inputs; never modified."""
    key = (case.key(), rounding, dtype)
    if key not in _REFS:
        with torch.no_grad():
            _REFS[key] = case.model(inputs_of(case), rounding=rounding, dtype=dtype)
    return _REFS[key]


def bf16_row_figures(case, got=None):
    """Per output of a bf16 row: the figures of the bf16 criterion (``got`` None: the model in fp32 stands in)."""
    ex, m64, m32 = (reference(case, r, d) for r, d in ((SR.EXACT, torch.float64), (SR.BF16, torch.float64),
                                                       (SR.BF16, torch.float32)))
    return [SR.bf16_figures(m32[j] if got is None else got[j], ex[j], m64[j], m32[j]) for j in range(len(ex))
            if got is None or got[j] is not None]


def check(case, dev):
    """Run one case -> (figures per output, violations).  Asserts the variant selection itself."""
    outs, names = case.run(inputs_of(case), dev)
    assert names == case.want, "the shape selects %s, the row is meant for %s" % (names, case.want)
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
