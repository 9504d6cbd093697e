"""What csrc/sampling.hip launches for a sampler call, on the host: furthest_point_sampling_plan_query (fps_plan(), which every
launcher of the file asks) against the case table of tests/fps_cases.py.  The table must name the form of every case, reach
every form any argument combination selects (a sweep of the query over n = 1..24576, the large-cloud boundaries and the slab
sampler's range), stand on both sides of every boundary, reach the forms behind the PWCLO_FPS_* switches, and the refusals
must carry the launchers' messages.  No GPU: the query is pure host code.
"""
import pytest

import fps_cases as T
from pwclonet_pylidarslam_amd import fused, preprocess
from pwclonet_pylidarslam_amd.pointnet2_ops import _ext as E


@pytest.mark.parametrize("case", T.ALL_CASES + T.SLAB_REFUSED, ids=T.case_id)
def test_every_case_names_its_form(case):
    plan = T.plan_of(case)
    assert T.forms(plan, case.chain) == case.want, (case, plan)


def test_table_reaches_every_reachable_form():
    """Default environment (capturing is an argument of a call, not a switch): the table's forms are exactly the sweep's."""
    can = T.reachable("default")
    reached = set()
    for c in T.ALL_CASES:
        if c.switches in ("default", "capturing", "order_torch"):
            reached.update(c.want)
    print("\nreachable sampler forms under the default environment: %d\n  %s" % (len(can), "\n  ".join(sorted(can))))
    assert reached == can, ("not reached", sorted(can - reached), "not selectable", sorted(reached - can))
    assert len(can) == 29
    want = {T.reg(*row, 1) for row in T.ROW_RANGES} | {T.reg(512, 0, 48, 0), T.reg(512, 0, 16, 0), T.STREAM, T.slab(16), T.slab(18),
                                                       "reg+tie_out", "reg+prefix_in", "reg+both", "slab+tie_out"}
    want |= {T.coop(o, r, l) for o in (0, 1) for r in (">=8", "<8") for l in ("cooperative", "plain")}
    assert can == want
    # run on the GPU, not only planned: every form but the plain launches of a capturing stream and the plain order at G >= 29
    ran = set()
    for c in T.ALL_CASES:
        if c.switches == "default" and (c.run or c.name == "large-n25000-b9"):
            ran.update(c.want)
    assert can - ran == {T.coop(o, r, "plain") for o in (0, 1) for r in (">=8", "<8")} | {T.coop(0, "<8")}


def test_switch_sets_reach_their_forms():
    """Each child set's cases select forms the set can select, among them every form only the set reaches; the plain-launch
    forms and the streaming kernel are the same kernels the default environment reaches by other arguments."""
    default = T.reachable("default")
    for name in T.CHILD_SETS:
        can = T.reachable(name)
        reached = set()
        for c in T.SWITCH_CASES:
            if c.switches == name:
                reached.update(c.want)
        assert reached and reached <= can, (name, sorted(reached - can))
        assert can - default <= reached, (name, sorted(can - default - reached))
        print("\n%s: %d forms, %d of them only under the switch; cases reach %s" % (name, len(can), len(can - default), sorted(reached)))
    assert T.reachable("table0") - default == {T.reg(256, 1, 8, 0)}
    assert {c.want for c in T.SWITCH_CASES if c.switches == "coop0"} == {(T.STREAM,)}
    assert {c.want for c in T.SWITCH_CASES if c.switches == "launch0"} == {(T.coop(0, ">=8", "plain"),)}
    assert all("fps_coop" not in f for f in T.reachable("coop0"))
    assert all(p["xcd_local"] == 0 for p in (T.plan_of(c) for c in T.SWITCH_CASES if c.switches == "launch0"))
    assert E.furthest_point_sampling_plan(1, 40000, 8)["xcd_local"] == 1
    assert E.furthest_point_sampling_plan(1, 40000, 8)["order"] == E.LARGE_CLOUD_ORDER
    assert E.furthest_point_sampling_plan(1, 40000, 8, order="torch")["order"] == "torch"


def test_both_sides_of_every_boundary_are_in_the_table():
    ns = {}
    for c in T.ALL_CASES + T.SLAB_REFUSED:
        ns.setdefault(c.entry, set()).add(c.n)
    single = ns["auto"] | ns["plain"]
    for row, (lo, hi) in T.ROW_RANGES.items():
        assert lo in ns["auto"] and hi in ns["auto"], row
        for n, other in ((lo, lo - 1), (hi, hi + 1)):                       # they ARE the boundaries: the neighbour is another form
            mine = E.furthest_point_sampling_plan(1, n, 8)
            assert (mine["T"], mine["E"], mine["I"]) == row
            if 1 <= other <= T.SMALL_CLOUD:
                o = E.furthest_point_sampling_plan(1, other, 8)
                assert (o["T"], o["E"], o["I"]) != row
    for lo, hi in ((T.TABLE_LAST_N, T.TABLE_LAST_N + 1),) + T.LARGE_BOUNDARIES:
        assert lo in single and hi in single, (lo, hi)
        a, b = (T.forms(E.furthest_point_sampling_plan(1, n, 8)) for n in (lo, hi))
        assert a != b, (lo, hi, a)
    for lo, hi in T.SLAB_BOUNDARIES:
        assert lo in ns["slab"] and hi in ns["slab"], (lo, hi)
        a, b = (T.forms(E.furthest_point_sampling_plan(1, n, 8, entry="slab")) for n in (lo, hi))
        assert a != b, (lo, hi, a)
    # G = 28 | 29 is the per-launch boundary, G = 32 | 33 the cooperative sampler's last cloud
    assert [E.furthest_point_sampling_plan(1, n, 8)["per_launch"] for n in (458752, 458753)] == [8, 7]
    assert [E.furthest_point_sampling_plan(1, n, 8)["G"] for n in (458752, 458753, 524288)] == [28, 29, 32]
    assert [E.furthest_point_sampling_plan(1, n, 8)["grid"] for n in (458752, 458753, 524288)] == [224, 232, 256]


def test_plan_fields_of_the_cooperative_launches():
    """per_launch = 224 / G in whole groups of 8 clouds from 8 on; the grid is padded to 8 clouds; the spatial order brings
    64 KiB of LDS; a capturing stream, or the switch, takes the plain launch."""
    for b, n in ((1, 24577), (9, 25000), (16, 120000), (3, 262144), (9, 458752), (8, 458753), (1, 524288)):
        for capturing in (False, True):
            p = E.furthest_point_sampling_plan(b, n, 8, capturing=capturing)
            G = -(-n // T.COOP_POINTS)
            per = 224 // G
            per = per & ~7 if per >= 8 else per
            assert (p["kernel"], p["G"], p["per_launch"], p["launches"]) == ("coop", G, per, -(-b // per)), p
            assert p["grid"] == 8 * G * -(-min(b, per) // 8) and p["grid"] <= 256
            assert p["sorted"] == (n >= T.SORTED_CLOUD) and p["lds_bytes"] == (65536 if p["sorted"] else 0)
            assert p["launch"] == ("plain" if capturing else "cooperative")
            assert (p["bs"], p["log2bs"], p["T"], p["I"]) == (512, 9, 1024, 16)
    assert E.furthest_point_sampling_plan(1, 40000, 8, coop_launch=0)["launch"] == "plain"
    assert E.furthest_point_sampling_plan(1, 40000, 8, use_sorted=0)["sorted"] == 0
    assert E.furthest_point_sampling_plan(1, 40000, 8, entry="plain")["sorted"] == 0
    # what cannot run cooperatively streams: too many workgroups, the switch, a temp that is not 8-byte aligned
    for kw in (dict(n=524289), dict(n=40000, use_coop=0), dict(n=40000, temp_aligned=False), dict(n=(1 << 23) - 1)):
        n = kw.pop("n")
        for entry in ("auto", "plain"):
            p = E.furthest_point_sampling_plan(3, n, 8, entry=entry, **kw)
            assert (p["kernel"], p["T"], p["grid"], p["lds_bytes"], p["sorted"]) == ("stream", 1024, 3, 0, 0), p


def test_plan_fields_of_the_single_workgroup_kernels():
    """LDS = 64 bytes of slots + the point table (when it fits: 160 KiB, 64 KiB with PWCLO_FPS_TABLE=0) + 8 bytes per logged
    decision; the row is the text-derived rule's (tests/test_host_cpu.py) for every n."""
    from oracle import ops as O
    for n in range(1, T.SMALL_CLOUD + 1):
        p = E.furthest_point_sampling_plan(2, n, 8)
        assert p["kernel"] == "reg" and (p["T"], p["E"], p["I"]) == T.row_of(n) and p["grid"] == 2, (n, p)
        assert p["table"] == (n <= T.TABLE_LAST_N) and p["lds_bytes"] == (64 + 16 * n if p["table"] else 64), (n, p)
        if n % 97 == 0 or n < 600:
            assert p["bs"] == O.opt_n_threads(n) and 1 << p["log2bs"] == p["bs"]
    for n, ti, table in ((8188, 4094, 1), (8189, 4094, 0), (10235, 1, 0), (10234, 1, 1), (4092, 0, 1)):
        p = E.furthest_point_sampling_plan(2, n, 8, entry="plain", tie_out=ti > 0, tie_iters=ti)
        log = 8 * (ti + 2) if ti else 0
        assert p["table"] == table and p["lds_bytes"] == 64 + log + (16 * n if table else 0), (n, ti, p)
    assert E.furthest_point_sampling_plan(2, 4093, 8, use_table=0)["table"] == 0
    assert E.furthest_point_sampling_plan(2, 4092, 8, use_table=0)["table"] == 1
    assert E.furthest_point_sampling_plan(2, 3273, 8, entry="plain", tie_out=True, tie_iters=1636, use_table=0)["table"] == 1
    assert E.furthest_point_sampling_plan(2, 3274, 8, entry="plain", tie_out=True, tie_iters=1636, use_table=0)["table"] == 0
    for n in (4096, 5000, 8192, 8193, 9216):
        p = E.furthest_point_sampling_plan(4, n, 8, entry="slab", tie_out=True, tie_iters=100)
        assert (p["kernel"], p["T"], p["I"], p["grid"]) == ("slab", 512, 16 if n <= 8192 else 18, 4)
        assert p["lds_bytes"] == 64 + 16 * n + 8 * 102
    assert E.furthest_point_sampling_plan(1, 9216, 8, entry="slab", tie_out=True, tie_iters=2048)["kernel"] == "refused"


@pytest.mark.parametrize("entry,n,kw,piece", T.REFUSED_CASES, ids=lambda v: str(v) if not isinstance(v, dict) else "")
def test_refusals_carry_the_launchers_messages(entry, n, kw, piece):
    p = E.furthest_point_sampling_plan(2, n, 8, entry=entry, **kw)
    assert p["kernel"] == "refused" and piece in p["message"], p
    assert all(p[k] == 0 for k in ("T", "G", "grid", "lds_bytes"))


def test_plan_query_python_wrapper_and_arguments():
    with pytest.raises(ValueError):
        E.furthest_point_sampling_plan(0, 100, 8)                # the launchers return at once: nothing to plan
    with pytest.raises(ValueError):
        E.furthest_point_sampling_plan(1, 100, 0)
    with pytest.raises(KeyError):
        E.furthest_point_sampling_plan(1, 100, 8, entry="other")
    p = E.furthest_point_sampling_plan(1, 100, 8)
    assert set(p) == set(E._FPS_PLAN_FIELDS) | {"order"} and p["launch"] is None and p["order"] is None
    assert E._fps_route(8192, True) == ("reg", False) and E._fps_route(40000, True) == ("coop", True)
    assert E._fps_route(40000, False) == ("coop", False) and E._fps_route(524289, True) == ("stream", False)


def test_python_constants_agree_with_the_plan():
    """preprocess.py and fused.py restate five limits of the dispatch for their buffer sizes and their host-side refusals:
    each equals the boundary the plan query shows."""
    def kernel(n, **kw):
        return E.furthest_point_sampling_plan(1, n, 8, **kw)
    assert kernel(preprocess._SMALL_CLOUD)["kernel"] == "reg" and kernel(preprocess._SMALL_CLOUD + 1)["kernel"] == "coop"
    assert kernel(preprocess._SORTED_CLOUD - 1)["sorted"] == 0 and kernel(preprocess._SORTED_CLOUD)["sorted"] == 1
    for n in (24577, 32768, 32769, 120000, 458752, 458753, 524288):
        p = kernel(n, capturing=True)
        assert p["G"] == -(-n // preprocess._COOP_POINTS) and p["per_launch"] == preprocess.sampler_max_clouds(n), (n, p)
        assert p["per_launch"] == (lambda per: per & ~7 if per >= 8 else per)(preprocess._COOP_PLAIN_WGS // p["G"])
    assert preprocess.sampler_max_clouds(preprocess._SMALL_CLOUD) is None
    last = preprocess._COOP_POINTS * preprocess._COOP_MAX_G
    assert kernel(last)["G"] == preprocess._COOP_MAX_G and kernel(last + 1)["kernel"] == "stream"
    assert preprocess.SWEEP_CAPACITY_LIMIT == last + 1
    assert kernel(last, entry="sorted")["kernel"] == "coop" and kernel(preprocess.SWEEP_CAPACITY_LIMIT, entry="sorted")["kernel"] == "refused"
    assert fused.FPS_CHAIN_INTS == 12
