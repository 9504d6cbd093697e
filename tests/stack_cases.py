"""The case table of tests/test_gpu_stack_variants.py, with its inputs and float64 references, shared with
tests/test_stack_plan_cpu.py, which runs every row as a dry run on CPU tensors, and tests/test_stack_reference_cpu.py.

A row names, in launch order, the kernel instantiation(s) it is meant to reach (``want``), as rocprofv3 prints them:
defaulted template arguments included.  Nothing here predicts the dispatch of csrc/fused_layers.hip, fused_hoisted.hip
or fused_sa.hip: both tests run the row inside ``_lib.launches()`` and compare ``want`` with what the library's launch
layer recorded (``launched``).  The comments beside the rows say why a shape sits where it does.

``Case.inputs(shapes_only=True)`` leaves the neighbour search out (index lists of the right shape, all zero): enough for
a dry run, which never reads them.  Everything here is CPU torch / numpy until ``run`` moves the inputs to its device.
"""
import numpy as np
import torch

import stack_reference as SR
from oracle import ops as O
from oracle import params
from pwclonet_pylidarslam_amd import _lib, fused
from pwclonet_pylidarslam_amd.pointnet2_ops.pointnet2_modules import PointnetFPModulePWCLONet, PointnetSAModulePWCLONet
from pwclonet_pylidarslam_amd.pwclonet import CostVolume, FlowPredictor

F32, BF3, B16 = "f32", "bf16x3", "bf16"
WFMT = {F32: fused.WFMT_F32, BF3: fused.WFMT_BF16X3, B16: fused.WFMT_BF16}
# read once per process by the library: CHILD_CASES run in ONE fresh child process with these set
CHILD_ENV = {"PWCLO_FL_WIDE": "0", "PWCLO_COARSE_W4": "0", "PWCLO_LANE6": "0", "PWCLO_LANE_UP": "0"}


def filled(module, prefix):
    sd = module.state_dict()
    for k, v in sd.items():
        v.copy_(torch.from_numpy(np.array(params.fill_value(prefix + "." + k, v.shape))).reshape(v.shape).to(v.dtype))
    return module.eval()


def cloud(seed, b, n, scale=10.0):
    return (torch.rand(b, n, 3, generator=torch.Generator().manual_seed(seed)) * 2 - 1) * scale


def randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def neighbours(k, xyz, query, shapes_only):
    if shapes_only:
        return torch.zeros(query.shape[0], query.shape[1], k, dtype=torch.int32)
    return O.knn_point_with_dist(k, xyz, query)[1]


class Case:
    """One table row.  ``want``: the kernel instantiation(s) the row is meant to reach; ``fmt``: weight format;
    ``setenv``: variables fused.py reads per call or at pack time (monkeypatch reaches those).  ``run(inputs, dev)``
    returns the outputs (None: an output the row does not compare)."""
    kind = ""

    def __init__(self, want, fmt=F32, setenv=None, **shape):
        self.want = [want] if isinstance(want, str) else list(want)
        self.fmt, self.setenv, self.shape = fmt, dict(setenv or {}), shape
        self.__dict__.update(shape)

    @property
    def id(self):
        # sa_h_kernel without its defaulted ninth argument: the ids the rows have always had
        first = self.want[0][:-len(", false>")] + ">" if self.want[0].count(",") == 8 and self.want[0].endswith(
            ", false>") else self.want[0]
        return "-".join([first.replace(" ", ""), self.fmt, "x".join(
            str(v).replace(" ", "") for v in self.shape.values() if isinstance(v, (int, tuple)))] + list(self.setenv))

    def key(self):                                  # what the inputs and the exact references depend on
        return (self.kind, tuple(sorted((k, str(v)) for k, v in self.shape.items())))


class Pointwise(Case):
    kind = "pointwise"

    def inputs(self, shapes_only=False):
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
        if i["tail"] is None:
            return (pw(*srcs),)
        job = fused.LinearJob(i["tail"][0].to(dev), i["tail"][1].to(dev))
        assert pw.tail_supported(job)
        return pw.with_tail(job, *srcs)


class SetAbstraction(Case):
    kind = "sa"

    def inputs(self, shapes_only=False):
        b, n, s, k, c = self.b, self.n, self.s, self.k, self.mlp[0]
        mod = filled(PointnetSAModulePWCLONet(mlp=list(self.mlp), npoint=s, nsample=k), self.name)
        xyz = cloud(1, b, n)
        new_xyz = xyz[:, :s].contiguous() + 0.01
        return dict(mod=mod, xyz=xyz, new_xyz=new_xyz, feat=randn(2, b, n, c) if c else None,
                    idx=neighbours(k, xyz, new_xyz, shapes_only))

    def model(self, i, **kw):
        return (SR.set_abstraction(i["mod"], i["xyz"], i["new_xyz"], i["feat"], i["idx"], **kw),)

    def run(self, i, dev):
        fsa = fused.FusedSAHoisted(i["mod"].to(dev))
        assert fsa.wfmt == WFMT[self.fmt]
        pre = fused.run_linear_jobs(fsa.jobs(i["feat"].to(dev)))[0] if i["feat"] is not None else None
        assert pre is None or (pre.dtype == torch.bfloat16) == (self.fmt == B16)
        return (fsa(i["xyz"].to(dev), i["new_xyz"].to(dev), pre, i["idx"].to(dev)),)


def _upconv_module(name, c2):
    return filled(PointnetFPModulePWCLONet(nsample=8, mlp=[64, 128, 64], post_mlp=[64 + c2, 64], radius=0.2, knn=True,
                                           use_xyz=True, bn=True), name)


class Upconv(Case):
    """Hoisted set-upconv + its post-MLP as separate launches; ``hoist=False``: the un-hoisted kernel."""
    kind = "upconv"

    def inputs(self, shapes_only=False):
        b, n2, n1, k, c2 = self.b, self.s, self.n, self.k, self.c2
        xyz2, xyz1 = cloud(3, b, n2), cloud(4, b, n1)
        return dict(mod=_upconv_module("pose_warp_refinement_2.setupconv_features", c2), xyz2=xyz2, xyz1=xyz1,
                    f2=randn(5, b, n2, c2), f1=randn(6, b, n1, 64), idx=neighbours(k, xyz1, xyz2, shapes_only))

    def model(self, i, **kw):
        return (SR.set_upconv(i["mod"], i["xyz2"], i["xyz1"], i["f2"], i["f1"], i["idx"], **kw),)

    def run(self, i, dev):
        g = {k_: v.to(dev) for k_, v in i.items() if k_ != "mod"}
        if not self.shape.get("hoist", True):
            up = fused.FusedUpconv(i["mod"].to(dev))
            return (up(g["xyz2"], g["xyz1"], g["f2"], g["f1"], g["idx"]),)
        up = fused.FusedUpconvHoisted(i["mod"].to(dev))
        assert up.wfmt == WFMT[self.fmt]
        (pre,) = fused.run_linear_jobs(up.jobs(g["f1"]))
        return (up(g["xyz2"], g["xyz1"], g["f2"], pre, g["idx"]),)


class UpconvPost(Case):
    """Both set-upconvs of a level and their post-MLPs as one launch."""
    kind = "upconv_post"
    NAMES = ["pose_warp_refinement_2.setupconv_features", "pose_warp_refinement_2.setupconv_mask"]

    def inputs(self, shapes_only=False):
        b, n2, n1, k, c2 = self.b, self.s, self.n, self.k, self.c2
        xyz2, xyz1 = cloud(3, b, n2), cloud(4, b, n1)
        return dict(mods=[_upconv_module(nm, c2) for nm in self.NAMES[:self.njobs]], xyz2=xyz2, xyz1=xyz1,
                    f2=randn(5, b, n2, c2), f1s=[randn(6 + j, b, n1, 64) for j in range(self.njobs)],
                    idx=neighbours(k, xyz1, xyz2, shapes_only))

    def model(self, i, **kw):
        return tuple(SR.set_upconv(m, i["xyz2"], i["xyz1"], i["f2"], f1, i["idx"], **kw)
                     for m, f1 in zip(i["mods"], i["f1s"]))

    def run(self, i, dev):
        ups = [fused.FusedUpconvHoisted(m.to(dev)) for m in i["mods"]]
        pres = fused.run_linear_jobs([u.jobs(f1.to(dev))[0] for u, f1 in zip(ups, i["f1s"])])
        return tuple(fused.run_upconv_post(ups, i["xyz2"].to(dev), i["xyz1"].to(dev), i["f2"].to(dev), pres,
                                           i["idx"].to(dev)))


class CostVol(Case):
    """The whole cost volume (first aggregate a1 + a2, then b); compared on ``first`` and on the result.
    ``hoist=False``: the un-hoisted kernels."""
    kind = "cv"

    def inputs(self, shapes_only=False):
        b, s, n, c, kq = self.b, self.s, self.n, self.c, self.kq
        mod = filled(CostVolume(nsample=4, nsample_q=kq, in_channel1=c, in_channel2=c, mlp1=[128, 64, 64],
                                mlp2=[128, 64]), "cost_volume")
        x1, x2 = cloud(7, b, s), cloud(8, b, n)
        return dict(mod=mod, x1=x1, x2=x2, p1=randn(9, b, s, c), p2=randn(10, b, n, c),
                    idx_q=neighbours(kq, x2, x1, shapes_only), idx=neighbours(4, x1, x1, shapes_only))

    def model(self, i, **kw):
        return SR.cost_volume(i["mod"], i["x1"], i["p1"], i["x2"], i["p2"], i["idx_q"], i["idx"],
                              hoisted=self.shape.get("hoist", True), **kw)

    def run(self, i, dev):
        g = {k_: v.to(dev) for k_, v in i.items() if k_ != "mod"}
        kp = fused.cv_pix_slots(self.kq)
        if not self.shape.get("hoist", True):
            cv = fused.FusedCostVolume(i["mod"].to(dev))
            assert cv.wfmt_a2 == fused.cv_stack_wfmt(kp, WFMT[self.fmt], hoisted=False)
            return cv(g["x1"], g["p1"], g["x2"], g["p2"], idx_q=g["idx_q"], idx=g["idx"]), None
        cv = fused.FusedCostVolumeHoisted(i["mod"].to(dev))
        assert cv.wfmt == fused.cv_stack_wfmt(kp, WFMT[self.fmt]) and cv.job_u.out_bf16 == (cv.wfmt == fused.WFMT_BF16)
        u, v, u2 = fused.run_linear_jobs(cv.jobs(g["p1"], g["p2"]))
        seen, second = {}, cv._second

        def keep(xyz1, u2_, v2, first, idx):       # cv_b's inputs: the first aggregate is compared too
            seen["first"], seen["v2"] = first, v2
            return second(xyz1, u2_, v2, first, idx)
        cv._second = keep
        out = cv(g["x1"], g["x2"], u, v, u2, idx_q=g["idx_q"], idx=g["idx"])
        assert seen["v2"].dtype == (torch.bfloat16 if cv.wfmt == fused.WFMT_BF16 else torch.float32)
        return out, seen["first"]


class Linear(Case):
    """linear_jobs with bf16 rows: every job once with fp32 rows and once with bf16 rows in ONE launch."""
    kind = "linear"
    JOBS = [(16, 128, 500), (32, 64, 33), (64, 128, 2051), (64, 16, 7)]

    def inputs(self, shapes_only=False):
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
        if dev.type != "cpu":                      # a dry run leaves the outputs unwritten
            for f32, b16 in zip(outs[0::2], outs[1::2]):
                assert b16.dtype == torch.bfloat16 and torch.equal(b16, f32.to(torch.bfloat16))      # bit for bit
        return tuple(outs[0::2])


PW_SETS = [((64, 64), [64]), ((64, 32), [64]), ((64, 16), [64]), ((64, 64, 64), [128, 64]), ((32, 64, 64), [128, 64]),
           ((64, 64, 32), [128, 64]), ((16, 64, 64), [128, 64]), ((128, 64), [128, 64])]      # fused_layers.hip PW_CASE
SA_SETS = [("psa_1", [0, 8, 8, 16], 20, "sa_h_kernel<1, 1, 1, 32, 2, 8, true, 0, true>", {}),
           ("psa_1", [0, 8, 8, 16], 20, "sa_h_kernel<1, 1, 1, 32, 2, 8, true, %d, false>", {"PWCLO_SA_KMAJOR": "0"}),
           ("psa_2", [16, 16, 16, 32], 20, "sa_h_kernel<1, 1, 2, 32, 2, 8, false, %d, false>", {}),
           ("psa_3", [32, 32, 32, 64], 11, "sa_h_kernel<2, 2, 4, 16, 1, 16, false, %d, false>", {}),
           ("psa_4", [64, 64, 64, 128], 11, "sa_h_kernel<4, 4, 8, 16, 1, 16, false, %d, false>", {})]


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
            t.append(SetAbstraction("sa_h_kernel<8, 4, 4, 16, 1, %d, false, %d, false>" % (w, WFMT[fmt]), fmt,
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
    SetAbstraction("sa_h_kernel<8, 4, 4, 16, 1, 16, false, 0, false>", name="flow_feature_encoding", mlp=[64, 128, 64, 64],
                   b=3, n=700, s=64, k=11),                                      # small, now 16 waves
]


# ---- inputs, references, and what a row launched ---------------------------------------------------------------------

_INPUTS, _REFS = {}, {}


def inputs_of(case, shapes_only=False):
    key = (case.key(), shapes_only)
    if key not in _INPUTS:
        _INPUTS[key] = case.inputs(shapes_only)
    return _INPUTS[key]


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


def launched(case, dev, dry=False):
    """Runs the row on ``dev`` -> (outputs, launch records of ``_lib.launches()`` in launch order).  The one filter:
    the hoisted rows' linear_jobs launches, kept only for the ``Linear`` row."""
    with _lib.launches(dry=dry) as rec:
        outs = case.run(inputs_of(case, shapes_only=dry), dev)
    return outs, [r for r in rec if case.kind == "linear" or r[1] != "linear_jobs_kernel"]
