"""Every furthest-point-sampling form of csrc/sampling.hip against the C oracle, bit for bit (run with ``-m gpu``).

Each case of tests/fps_cases.py first asserts through furthest_point_sampling_plan_query -- the launchers' own fps_plan() --
that its call selects the form it is meant for, runs its entry point and requires the indices to be ``torch.equal`` to
``oracle.ops.furthest_point_sampling`` and the sampled coordinates, where the entry writes them, to be the gathered points bit
for bit.  All outputs are integers or copied coordinates: there is no tolerance anywhere.  tests/test_fps_plan_cpu.py proves
that the table reaches every form the dispatch can select.
"""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import fps_cases as T
from pwclonet_pylidarslam_amd import _lib, fused
from pwclonet_pylidarslam_amd.pointnet2_ops import _ext as E

pytestmark = pytest.mark.gpu


def assert_plan(case):
    plan = T.plan_of(case)
    assert T.forms(plan, case.chain) == case.want, (case.name, plan)
    return plan


def check(case, x, idx, new_xyz, want):
    assert torch.equal(idx.cpu(), want), "%s: %d indices differ from the oracle" % (case.name, int((idx.cpu() != want).sum()))
    if new_xyz is not None:
        assert torch.equal(T.bits(new_xyz.cpu()), T.bits(T.gathered(x, want))), case.name


# ---- 1. every reg form x cloud kinds ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reg_reference(n):
    """The batch of the five cloud kinds and the oracle's n + 3 samples: every shorter call is a prefix of them."""
    case = next(c for c in T.REG_CASES if c.n == n)
    x = T.make_batch(case)
    return x, T.oracle(x, n + 3)


@pytest.mark.parametrize("case", T.REG_CASES, ids=T.case_id)
def test_reg_forms_on_five_cloud_kinds(cuda, case):
    assert_plan(case)
    x, ref = _reg_reference(case.n)
    assert (ref[4] == 0).all() and len(torch.unique(ref[3])) <= 8          # no eligible point; at most 7 (and index 0)
    for m in T.reg_ms(case.n):
        want = ref[:, :m].contiguous()
        c = case._replace(m=m)
        check(c, x, *T.run(c, x, cuda), want)
        c = c._replace(entry="plain")                                       # the same kernel writing the coordinates too
        check(c, x, *T.run(c, x, cuda), want)


# ---- 2. chain forms ----------------------------------------------------------------------------------------------------------------
def _records(b, dev):
    return torch.full((b, fused.FPS_CHAIN_INTS), -1, dtype=torch.int32, device=dev)


@pytest.mark.parametrize("last", [False, True], ids=["record", "last-decision"])
@pytest.mark.parametrize("cc", T.CHAIN_CASES, ids=T.case_id)
def test_chain_records_and_prefix_children(cuda, cc, last):
    tag = "-last" if last else ""
    by_name = {c.name: c for c in T.CHAIN_PLAN_CASES}
    parent = by_name[cc.name + tag + "-parent"]
    ti = parent.chain.tie_iters
    assert_plan(parent)
    x = T.make_chain_batch(cc, last)
    rec = _records(parent.b, cuda)
    idx0, s0 = T.run(parent, x, cuda, tie_out=rec)
    check(parent, x, idx0, s0, T.oracle(x, parent.m))
    r = rec.cpu()
    print("\n%s: records %s" % (parent.name, r[:, :2 + T.MANY_TIES_PAIRS].tolist()))
    if last:                                            # four beacons, then the pair: one event, at the last recorded decision
        for b in range(parent.b):
            assert r[b, :3].tolist() == [0, 1, ti - 1], (b, r[b])
    else:
        tiefree, one, many = r[0], r[1], r[2]
        assert one[0].item() in (0, 1) and many[0].item() == 1            # more than eight events: the fallback flag
        if one[0].item() == 0:                                             # (a chance tie of the background may raise it)
            assert one[1].item() >= 1 and 1 in one[2:2 + int(one[1])].tolist()
    samples = s0.cpu().contiguous()
    for m in sorted({ti, 1}):
        child = by_name["%s%s-child-m%d" % (cc.name, tag, m)]
        assert_plan(child)
        want = T.oracle(samples, m)                     # the oracle's FULL sampling of the parent's samples
        idx1, s1 = T.run(child, samples, cuda, prefix_in=rec)
        check(child, samples, idx1, s1, want)
        if not last and m == ti and r[0, 0].item() == 0 and r[0, 1].item() == 0:
            assert torch.equal(idx1[0].cpu(), torch.arange(m, dtype=torch.int32))      # no tie at all: the prefix itself
    both = by_name[cc.name + tag + "-child-both"]
    assert_plan(both)
    rec2 = _records(both.b, cuda)
    idx2, s2 = T.run(both, samples, cuda, tie_out=rec2, prefix_in=rec)
    check(both, samples, idx2, s2, T.oracle(samples, both.m))


@pytest.mark.parametrize("name", ["chain-table-flip-8192", "chain-table-keep-8188"])
def test_chain_log_moves_the_point_table(cuda, name):
    """The longest record a pyramid asks for (tie_iters = n / 2) pushes the point table of n >= 8189 out of LDS."""
    case = next(c for c in T.CHAIN_PLAN_CASES if c.name == name)
    assert_plan(case)
    x = T.make_batch(case)
    rec = _records(case.b, cuda)
    idx, new_xyz = T.run(case, x, cuda, tie_out=rec)
    check(case, x, idx, new_xyz, T.oracle(x, case.m))
    assert set(rec[:, 0].cpu().tolist()) <= {0, 1}


# ---- 3. large clouds ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in T.LARGE_CASES if c.run], ids=T.case_id)
def test_large_clouds(cuda, case):
    plan = assert_plan(case)
    if plan["kernel"] == "coop":
        assert plan["launch"] == "cooperative"
    x = T.make_batch(case)
    want = T.oracle(x, case.m)
    idx, new_xyz = T.run(case, x, cuda)
    _lib.synchronize(cuda)                              # a workgroup that timed out waiting for its peers raises here
    check(case, x, idx, new_xyz, want)


# ---- 4. the spatial order, directly ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", T.ORDER_BATCHES, ids=lambda k: k[0])
@pytest.mark.parametrize("n", T.ORDER_SIZES)
def test_spatial_order_kernels(cuda, n, kinds):
    b = len(kinds)
    x = torch.stack([T.make_cloud(k, 1 + i, n) for i, k in enumerate(kinds)]).contiguous()
    xd = x.to(cuda)
    lib = _lib.load()
    ws = torch.empty((lib.fps_spatial_order_workspace_bytes(b, n),), dtype=torch.uint8, device=cuda)
    sorted_pts = torch.full((b, n, 3), float("nan"), device=cuda)
    perm = torch.full((b, n), -1, dtype=torch.int32, device=cuda)
    _lib.call("fps_spatial_order_kernel_wrapper", cuda, b, n, xd.data_ptr(), sorted_pts.data_ptr(), perm.data_ptr(), ws.data_ptr())
    p = perm.cpu().long()
    assert torch.equal(p.sort(dim=1).values, torch.arange(n).expand(b, -1)), "perm is not a permutation"
    assert torch.equal(T.bits(sorted_pts.cpu()), T.bits(torch.gather(x, 1, p.unsqueeze(-1).expand(-1, -1, 3))))
    pri = E._fps_priorities(n, "cpu")[p]                                   # (b, n)
    rising = pri[:, 1:] > pri[:, :-1]
    inside = (torch.arange(1, n) % 1024) != 0                              # position pairs that do not straddle two blocks
    assert bool(rising[:, inside].all()), "a block of 1024 positions is not in strictly ascending priority"
    mag = (x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]) + x[..., 2] * x[..., 2]
    eligible = ~(mag.double() <= 1e-3)
    el = torch.gather(eligible, 1, p)
    count = eligible.sum(dim=1)
    # every never-eligible row behind every eligible row -- in whole blocks: the one block that holds the last eligible rows and
    # the first never-eligible ones is, like every block, in priority order, so inside it the two kinds interleave
    for i in range(b):
        full = int(count[i]) // 1024 * 1024
        assert bool(el[i, :full].all()) and not bool(el[i, full + 1024:].any()), (kinds[i], int(count[i]))
        assert int(el[i, full:full + 1024].sum()) == int(count[i]) - full
    m = 32
    tmp = torch.full((b, n), 1e10, device=cuda)
    idx = torch.zeros((b, m), dtype=torch.int32, device=cuda)
    new_xyz = torch.empty((b, m, 3), device=cuda)
    plan = E.furthest_point_sampling_plan(b, n, m, entry="sorted")
    assert T.forms(plan) == (T.coop(1, ">=8"),)
    _lib.call("furthest_point_sampling_sorted_kernel_wrapper", cuda, b, n, m, xd.data_ptr(), sorted_pts.data_ptr(), perm.data_ptr(),
              tmp.data_ptr(), idx.data_ptr(), new_xyz.data_ptr())
    _lib.synchronize(cuda)
    want = T.oracle(x, m)
    assert torch.equal(idx.cpu(), want)
    assert torch.equal(T.bits(new_xyz.cpu()), T.bits(T.gathered(x, want)))


# ---- 5. the slab sampler -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _slab_reference(n):
    case = next(c for c in T.SLAB_CASES if c.n == n)
    x = T.make_batch(case)
    return x, T.oracle(x, case.m)


@pytest.mark.parametrize("case", T.SLAB_CASES, ids=T.case_id)
def test_slab_sampler(cuda, case):
    assert_plan(case)
    x, want = _slab_reference(case.n)
    rec = _records(case.b, cuda) if case.chain.tie_out else None
    idx, new_xyz = T.run(case, x, cuda, tie_out=rec)
    check(case, x, idx, new_xyz, want)
    if rec is not None:                                 # the later level driven by the record equals the oracle's
        samples = new_xyz.cpu().contiguous()
        i1, s1 = fused.fps_with_xyz(new_xyz, case.chain.tie_iters, prefix_in=rec)
        ref1 = T.oracle(samples, case.chain.tie_iters)
        assert torch.equal(i1.cpu(), ref1) and torch.equal(T.bits(s1.cpu()), T.bits(T.gathered(samples, ref1)))
        assert set(rec[:, 0].cpu().tolist()) <= {0, 1} and rec[1, 0].item() == 1       # the lattice: ties everywhere


@pytest.mark.parametrize("case", T.SLAB_REFUSED, ids=T.case_id)
def test_slab_sampler_refuses_outside_its_range(cuda, case):
    plan = assert_plan(case)
    assert "outside the slab sampler's range" in plan["message"]
    x = T.make_batch(case)
    with _lib.launches() as seen:
        with pytest.raises(RuntimeError, match="outside the slab sampler's range"):
            fused.fps_slab_with_xyz(x.to(cuda), case.m)
    assert [s for s in seen if "fps_" in s[1]] == []    # nothing of the sampler was launched


# ---- 6. the switches -------------------------------------------------------------------------------------------------------------------
def test_switch_sets_in_child_processes(cuda):
    """Each PWCLO_FPS_* switch is read once per process, so each set runs in a fresh child (tests/fps_cases.py --child), one
    after the other, each with its own time limit; the next is not started after one that died.  A child asserts nothing: it
    prints the forms its plan query names -- from the explicit arguments and from its own environment -- and the number of
    differences from the oracle."""
    for name in T.CHILD_SETS:
        env = dict(os.environ, **T.SWITCH_SETS[name]["env"])
        try:
            out = subprocess.run([sys.executable, os.path.join(T.ROOT, "tests", "fps_cases.py"), "--child", name], env=env,
                                 cwd=T.ROOT, capture_output=True, text=True, timeout=150)
        except subprocess.TimeoutExpired:
            pytest.exit("the %s child hung: nothing more is started on this GPU" % name, returncode=3)
        if out.returncode < 0 or out.returncode in (134, 137, 139):        # killed by a signal: a fault, not a difference
            pytest.exit("the %s child died (%d): nothing more is started on this GPU\n%s"
                        % (name, out.returncode, out.stderr[-2000:]), returncode=3)
        assert out.returncode == 0, (name, out.returncode, out.stdout[-2000:], out.stderr[-2000:])
        got = json.loads(out.stdout.strip().splitlines()[-1])
        print("\n%s" % got)
        cases = [c for c in T.SWITCH_CASES if c.switches == name]
        assert got["set"] == name and set(got["results"]) == {c.name for c in cases}
        for c in cases:
            res = got["results"][c.name]
            assert tuple(res["forms"]) == c.want and tuple(res["env_forms"]) == c.want, (c.name, res)
            assert res["differences"] == 0, (c.name, res)
            if name == "launch0":
                assert res["xcd_local"] == 0
