"""Which csrc/conv1x1.hip instantiations the host dispatch can select, and that tests/test_gpu_conv_variants.py reaches
all of them: conv1x1_plan_query (the launchers' own conv_grid() / wgrad_plan(), host only) enumerated for 256 CUs over
the channel counts 1..512 and a ladder of pixel counts, against the case table of tests/conv_variant_cases.py.

A form of the forward family is (NBO, STATS, LEAN, transposed): the input-gradient entry points pack the weights through
the other path, so they count separately.  A form of the weight gradient is (RO, RM, ph, XF); the plan is the same with
and without the input transform XF, which the caller chooses.  Outputs of 4 GiB and more (the only way a plain forward
takes the general epilogue) are outside the ladder, as they are outside the GPU test.
"""
import ctypes

import pytest

import conv_variant_cases as T

CUS = 256
KINDS = ("forward", "dgrad", "stats", "dgrad_sums", "affine", "pooled")
TRANSPOSED = {"forward": 0, "dgrad": 1, "stats": 0, "dgrad_sums": 1, "affine": 0, "pooled": 0}
# b x p: 1 tile ... 2048 tiles, whole and ragged, across the thresholds of the few-pixel split (2^k x 128 tiles + 1)
LADDER = [(1, 4), (1, 32), (2, 36), (1, 256), (1, 288), (1, 2048), (1, 4096), (1, 4128), (1, 8192), (1, 8224), (1, 16384),
          (1, 16416), (1, 32768), (1, 32800), (3, 10936), (32, 2048)]
# conv_grid() sees the channel counts as 16-channel blocks: both ends of every block count (checked for every pair below)
REPS = sorted({16 * m - 15 for m in range(1, 33)} | {16 * m for m in range(1, 33)})


@pytest.fixture(scope="module")
def query():
    from pwclonet_pylidarslam_amd import _lib, conv1x1
    fn = _lib.load().conv1x1_plan_query
    out = (ctypes.c_int * 8)()

    def q(kind, b, cin, cout, p):
        rc = fn(conv1x1.PLAN_KINDS[kind], b, cin, cout, p, CUS, out)
        assert rc in (0, 1), (kind, b, cin, cout, p, rc)
        return rc == 0, tuple(out[:7 if kind == "wgrad" else 5])
    return q


@pytest.fixture(scope="module")
def reachable(query):
    """-> (forward-family forms, weight-gradient (ro, rm, ph)) that an ACCEPTED launch selects."""
    fwd, wg = set(), set()
    for b, p in LADDER:
        for cin in REPS:
            for cout in REPS:
                for kind in KINDS:
                    ok, (nbo, gy, gx, lean, stats) = query(kind, b, cin, cout, p)
                    if ok:
                        fwd.add((nbo, stats, lean, TRANSPOSED[kind]))
                ok, plan = query("wgrad", b, cin, cout, p)
                if ok:
                    wg.add(plan[:3])
    return fwd, wg


def test_plan_query_python_wrapper_and_arguments():
    from pwclonet_pylidarslam_amd import conv1x1
    assert conv1x1.plan("forward", 3, 192, 128, 2052, CUS) == dict(nbo=1, gy=8, gx=25, lean=1, stats=0, accepted=True)
    assert conv1x1.plan("forward", 3, 192, 128, 10936, CUS) == dict(nbo=8, gy=1, gx=129, lean=1, stats=0, accepted=True)
    assert conv1x1.plan("wgrad", 3, 192, 128, 10936, CUS) == dict(ro=4, rm=3, ph=1, wo=2, wm=4, cp=32, grid=256,
                                                                   accepted=True)
    assert conv1x1.plan("wgrad", 1, 160, 144, 64, CUS)["ro"] == 0 and not conv1x1.plan("wgrad", 1, 160, 144, 64, CUS)["accepted"]
    # the tile count from which a layer of <= 128 channels keeps all its blocks in one workgroup
    assert conv1x1.plan("forward", 1, 64, 128, 32 * 1024, CUS)["nbo"] == 4
    assert conv1x1.plan("forward", 1, 64, 128, 32 * 1025, CUS)["nbo"] == 8
    with pytest.raises(ValueError):
        conv1x1.plan("forward", 0, 16, 16, 64, CUS)
    with pytest.raises(ValueError):
        conv1x1.plan("forward", 1, 16, 16, 64, -1)


def test_forward_plan_depends_on_channel_blocks_only(query):
    """Every (cin, cout) in 1..512 gives the plan of the full blocks it rounds up to: the enumeration over REPS below
    stands for every pair."""
    b, p = T.UNSPLIT
    full = {(ci, co): query("forward", b, ci, co, p) for ci in range(16, 513, 16) for co in range(16, 513, 16)}
    for cin in range(1, 513):
        for cout in range(1, 513):
            assert query("forward", b, cin, cout, p) == full[(-(-cin // 16) * 16, -(-cout // 16) * 16)], (cin, cout)


def test_wgrad_split_mirror_agrees_with_the_plan(query):
    """conv1x1._wgrad_split (Python, part of ``supported``) says exactly where wgrad_plan() finds a rectangle."""
    from pwclonet_pylidarslam_amd import conv1x1
    seen = set()
    for cin in range(1, 513):
        for cout in range(1, 513):
            ok, (ro, rm, ph, wo, wm, cp, grid) = query("wgrad", 2, cin, cout, 260)
            assert bool(conv1x1._wgrad_split(cin, cout)) == (ro > 0), (cin, cout, ro)
            if ro > 0:
                assert ph * wo * wm == 8 and (ph == 1 or ro * rm == 1)
                assert wo * ro * 16 >= cout and wm * rm * 16 >= cin           # the workers' rectangles cover the tile grid
                seen.add((ro, rm, ph))
    assert {(ro, rm) for ro, rm, ph in seen} == {(ro, rm) for ro, rm, xf in T.INSTANTIATED_WGRAD}


def test_gpu_case_table_reaches_every_reachable_form(query, reachable):
    fwd, wg = reachable
    got_fwd, got_wg = set(), set()
    for c in T.CASES:
        ok, plan = query(c.entry, c.b, c.cin, c.cout, c.p)
        assert ok != bool(c.opts.get("refused")), T.case_id(c)
        if c.entry == "wgrad":
            assert plan[:3] == c.want, (T.case_id(c), plan)
            ro, rm, ph, wo, wm, cp, grid = plan
            chunks = c.b * -(-c.p // cp)
            chunk = c.opts.get("chunk")
            assert chunk != "walk" or (chunks > grid and c.p % cp != 0), (T.case_id(c), plan)
            assert chunk != "short" or (cp < c.p and c.p % cp != 0), (T.case_id(c), plan)
            assert chunk != "below" or c.p < cp, (T.case_id(c), plan)
            got_wg.add(plan[:3] + (c.opts["xf"],))
        else:
            nbo, gy, gx, lean, stats = plan
            assert (nbo, gy, lean, stats) == c.want, (T.case_id(c), plan)
            if ok:
                got_fwd.add((nbo, stats, lean, TRANSPOSED[c.entry]))
    want_wg = {f + (xf,) for f in wg for xf in (0, 1)}
    assert got_fwd == fwd, ("not reached", sorted(fwd - got_fwd), "not reachable", sorted(got_fwd - fwd))
    assert got_wg == want_wg, ("not reached", sorted(want_wg - got_wg), "not reachable", sorted(got_wg - want_wg))
    assert {c.opts.get("chunk") for c in T.CASES if c.entry == "wgrad"} >= {"walk", "short", "below"}
    # every instantiation is selectable, and nothing outside the instantiations is ever selected
    unreachable_fwd = T.INSTANTIATED_FORWARD - {f[:3] for f in fwd}
    unreachable_wg = T.INSTANTIATED_WGRAD - {(ro, rm, xf) for ro, rm, ph, xf in want_wg}
    print("\nconv1x1 forms reachable on %d CUs: %d of the forward family (x transposed: %d), %d weight-gradient "
          "(ro, rm, ph, xf); instantiated but unreachable below 4 GiB: %s %s"
          % (CUS, len({f[:3] for f in fwd}), len(fwd), len(want_wg), sorted(unreachable_fwd) or "none",
             sorted(unreachable_wg) or "none"))
    assert {f[:3] for f in fwd} <= T.INSTANTIATED_FORWARD
    assert {(ro, rm, xf) for ro, rm, ph, xf in want_wg} <= T.INSTANTIATED_WGRAD
    # the statistics-of-the-gradient epilogue exists for 1..4 blocks; a wider layer is refused, never launched as nothing
    assert all(nbo <= 4 for nbo, stats, lean, tr in fwd if stats == 2)
