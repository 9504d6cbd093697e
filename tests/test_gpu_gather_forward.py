"""The forward index-driven kernels -- group_points (dense and strided), gather_points, three_interpolate, the parts of the
concatenated stack input (geometry_encode, xyz_diff, broadcast_centre), three_nn and ball_query -- form by form and bit for
bit against host references (run with ``-m gpu``).

Every row of tests/gather_cases.py runs.  A group row first sets its launch settings through ``group_points_tuning``, asserts
through ``group_points_plan`` that the form it names is what will launch (tests/test_gather_plan_cpu.py proves the table
reaches every form the dispatch can produce), runs ``group_points`` and ``group_points_into`` on the source-identity and
the bit-pattern fill, and puts the settings back.  Outputs are compared as int32 words, so -0.0, infinities, subnormals and
NaN payloads count; the channels around a written slice must still hold the sentinel word.  The arithmetic outputs are
compared with numpy float32 arithmetic in the kernel's stated order, the search outputs with the CPU oracle.  No tolerances.
"""
import contextlib

import numpy as np
import pytest
import torch

import gather_cases as T
from oracle import ops as O
from pwclonet_pylidarslam_amd.pointnet2_ops import _ext as E

pytestmark = pytest.mark.gpu


def check(got, want, label, source=None):
    """Exact equality of int32 words; a mismatch names the first culprit (and, with the identity fill, the source element
    that arrived instead)."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.int32, (label, got.shape, want.shape)
    bad = np.argwhere(got != want)
    if len(bad) == 0:
        return
    at = tuple(int(v) for v in bad[0])
    msg = "%s: %d of %d words differ; first at %s: got 0x%08x, want 0x%08x" % (
        label, len(bad), got.size, at, int(got[at]) & 0xFFFFFFFF, int(want[at]) & 0xFFFFFFFF)
    if source is not None:
        b, c, n = source
        g, w = float(got[at].view(np.float32)), float(want[at].view(np.float32))
        if g == g and 0 <= g < b * c * n and g == int(g):
            msg += " -- source (b, c, i) = %s instead of %s" % (np.unravel_index(int(g), source), np.unravel_index(int(w), source))
    pytest.fail(msg)


def dev(a, cuda):
    """numpy int32 words -> fp32 device tensor of the same bits; other arrays as they are."""
    if a.dtype == np.int32:
        return T.as_f32(a).to(cuda)
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def dev_idx(idx, cuda, misalign=False):
    t = torch.from_numpy(np.ascontiguousarray(idx)).to(cuda)
    if misalign:                       # the same list 4 bytes into a larger buffer
        buf = torch.zeros(t.numel() + 1, dtype=torch.int32, device=cuda)
        buf[1:].copy_(t.reshape(-1))
        t = buf[1:].view(idx.shape)
    assert t.is_contiguous() and t.data_ptr() % 16 == (4 if misalign else 0)
    return t


@contextlib.contextmanager
def tuning(**tune):
    E.group_points_tuning(**tune)
    try:
        yield
    finally:
        E.group_points_tuning()


@pytest.mark.parametrize("case", T.GROUP_CASES, ids=T.case_id)
def test_group_points_every_form(cuda, case):
    b, c, n, s, k = case[:5]
    P = s * k
    misalign = case.opts.get("misalign", False)
    with tuning(**case.tune):
        plan = E.group_points_plan(b, c, n, P, aligned=not misalign)          # the settings as the launcher now reads them
        assert T.group_form(plan, P) == case.want, plan
        assert T.short_last_workgroup(plan, P) == case.opts.get("short_wg", False), plan
        for kind in T.FILLS:
            bits, idx = T.group_inputs(case, kind)
            want = T.ref_group(bits, idx)
            pts, idx_d = dev(bits, cuda), dev_idx(idx, cuda, misalign)
            assert pts.data_ptr() % 16 == 0
            source = (b, c, n) if kind == "identity" else None
            label = "%s %s %s" % (T.case_id(case), plan, kind)
            out = E.group_points(pts, idx_d)
            assert out.data_ptr() % 16 == 0
            check(T.bits_of(out), want, label + " dense", source)
            stack = dev(T.stack_of(b, c + 3, s, k), cuda)
            E.group_points_into(pts, idx_d, stack, 2)
            check(T.bits_of(stack), T.ref_stack(want, 2, 1), label + " strided")


def test_group_points_tuning_is_restored_and_defaults_launch(cuda):
    """After every row the process is back on its environment's settings: the plan without arguments is the default one (no
    switch is set under the suite), and a default launch gives the reference's bits."""
    case = next(c for c in T.GROUP_CASES if (c.c, c.n) == (3, 8192))
    plan = E.group_points_plan(case.b, case.c, case.n, case.s * case.k)
    import os
    if not any(v in os.environ for v in ("PWCLO_GROUP_LDS", "PWCLO_GP_THREADS", "PWCLO_GP_TARGET", "PWCLO_GP_NT")):
        assert plan == E.group_points_plan(case.b, case.c, case.n, case.s * case.k, **T.DEFAULT_TUNE)
        assert (plan["form"], plan["T"], plan["nt"]) == ("lds", 1024, 1)
    bits, idx = T.group_inputs(case, "bits")
    check(T.bits_of(E.group_points(dev(bits, cuda), dev_idx(idx, cuda))), T.ref_group(bits, idx), "level-0 grouping")


@pytest.mark.parametrize("case", T.GATHER_CASES, ids=T.case_id)
def test_gather_points(cuda, case):
    for kind in T.FILLS:
        bits, idx = T.gather_inputs(case, kind)
        got = E.gather_points(dev(bits, cuda), dev_idx(idx, cuda))
        check(T.bits_of(got), T.ref_gather(bits, idx), "%s %s" % (T.case_id(case), kind),
              (case.b, case.c, case.n) if kind == "identity" else None)


@pytest.mark.parametrize("case", T.INTERP_CASES, ids=T.case_id)
def test_three_interpolate(cuda, case):
    pts, idx, w = T.interp_inputs(case)
    got = E.three_interpolate(dev(pts, cuda), dev_idx(idx, cuda), dev(w, cuda))
    check(T.bits_of(got), T.ref_interp(pts, idx, w).view(np.int32), T.case_id(case))


@pytest.mark.parametrize("case", T.BCAST_CASES, ids=T.case_id)
def test_broadcast_centre(cuda, case):
    b, c, s, k, c_off = case
    for kind in T.FILLS:
        bits = T.bcast_inputs(case, kind)
        stack = dev(T.stack_of(b, c_off + c + 2, s, k), cuda)
        assert stack.data_ptr() % 16 == 0
        E.broadcast_centre_into(dev(bits, cuda), k, stack, c_off)
        check(T.bits_of(stack), T.ref_stack(T.ref_bcast(bits, k), c_off, 2), "%s %s" % (T.case_id(case), kind))


@pytest.mark.parametrize("case", T.GEO_CASES, ids=T.case_id)
def test_geometry_encode_and_xyz_diff(cuda, case):
    b, n, s, k = case
    for kind in T.FILLS + ("real",):
        centre, src, idx = T.geo_inputs(case, kind)
        args = (dev(centre, cuda), dev(src, cuda), dev_idx(idx, cuda))
        label = "%s %s" % (T.case_id(case), kind)
        stack = dev(T.stack_of(b, 1 + 10 + 2, s, k), cuda)
        E.geometry_encode_into(*args, stack, 1)
        got = T.bits_of(stack)
        if kind == "bits":             # NaNs and infinities: the six copied channels are the sources' bits; around them, sentinels
            check(got[:, :7], T.ref_stack(T.ref_geo_copies(centre, src, idx), 1, 0), label + " geometry copies")
            check(got[:, 11:], T.stack_of(b, 2, s, k), label + " geometry sentinels")
            continue
        check(got, T.ref_stack(T.ref_geo(centre, src, idx), 1, 2), label + " geometry")
        stack = dev(T.stack_of(b, 2 + 3 + 1, s, k), cuda)
        E.xyz_diff_into(*args, stack, 2)
        check(T.bits_of(stack), T.ref_stack(T.ref_xyz_diff(centre, src, idx).view(np.int32), 2, 1), label + " xyz_diff")


@pytest.mark.parametrize("case", T.THREE_NN_CASES, ids=T.case_id)
def test_three_nn(cuda, case):
    unknown, known = T.three_nn_inputs(case)
    want_d, want_i = O.three_nn(torch.from_numpy(unknown), torch.from_numpy(known))
    got_d, got_i = E.three_nn(dev(unknown, cuda), dev(known, cuda))
    check(got_i.cpu().numpy(), want_i.numpy(), T.case_id(case) + " indices")
    check(T.bits_of(got_d), T.bits_of(want_d), T.case_id(case) + " distances")


@pytest.mark.parametrize("case", T.BALL_CASES, ids=T.case_id)
def test_ball_query(cuda, case):
    q, xyz = T.ball_inputs(case)
    want = O.ball_query(torch.from_numpy(q), torch.from_numpy(xyz), T.BALL_RADIUS, case.nsample)
    got = E.ball_query(dev(q, cuda), dev(xyz, cuda), T.BALL_RADIUS, case.nsample)
    check(got.cpu().numpy(), want.numpy(), T.case_id(case))          # a query with no hit: the oracle's row, whatever the fill
