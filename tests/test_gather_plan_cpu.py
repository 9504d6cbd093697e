"""Which forms of the forward grouping kernels (csrc/group_points.hip: gp_forward) the host dispatch can select, and that
tests/test_gpu_gather_forward.py reaches all of them: group_points_plan_query (the launcher's own gp_forward_plan(), host
only) against the case table of tests/gather_cases.py and swept over a grid of shapes and settings.  Also, on the CPU: the
default settings still select the launch the dispatch made before it had a plan function, a thread count the kernel does
not exist for is sized for the 256 threads that run, and the host references of every table notice the faults a gather
kernel can have -- an unwritten tail, a shifted channel, a centre boundary off by one, a lost sign bit, a canonicalised
NaN.
"""
import ast
import itertools
import os

import numpy as np
import pytest
import torch

import gather_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "pwclonet_pylidarslam_amd", "csrc", "group_points.hip")


@pytest.fixture(scope="module")
def E():
    from pwclonet_pylidarslam_amd.pointnet2_ops import _ext
    return _ext


def legacy_launch(b, c, n, P, aligned=True, use_lds=1, threads=0, target=0, nt=1):
    """The launch gp_forward made before gp_forward_plan() existed, transcribed from that code: (kernel, T, nt, gx, per_wg,
    lds_bytes).  ``threads`` outside {1024, 512, 256} sized the grid from the value given and ran the 256-thread kernel."""
    cdiv = lambda a, d: -(-a // d)
    gy = cdiv(c, 8)
    vec = P % 4 == 0 and aligned
    need = min(c, 8) * n * 4
    if vec and use_lds and need <= 8 * 4096 * 4:
        T_ = threads if threads else 1024
        tgt = target if target else (512 if need < 64 * 1024 else 256)
        slices = b * gy
        gx = min(max(1, (tgt + slices - 1) // slices), cdiv(P, T_ * 4))
        per_wg = cdiv(cdiv(P, gx), T_ * 4) * T_ * 4
        return ("lds", T_ if T_ in (1024, 512) else 256, int(bool(nt)), cdiv(P, per_wg), per_wg, need)
    return ("direct_vec4", 256, 0, cdiv(P // 4, 256), 1024, 0) if vec else ("direct_scalar", 256, 0, cdiv(P, 256), 256, 0)


def launch_of(plan):
    return (plan["form"], plan["T"], plan["nt"], plan["gx"], plan["per_wg"], plan["lds_bytes"])


def test_plan_query_python_wrapper_arguments_and_setter(E):
    assert E.group_points_plan(1, 9, 64, 8196, threads=1024, target=1, nt=1, use_lds=1) == dict(
        form="lds", T=1024, nt=1, gx=1, per_wg=12288, lds_bytes=2048, staged_vec=1, tail=1)
    # c = 9 is two slices: target = 2 still means one workgroup per slice, 4 gives each slice two -- the second of 4 positions
    assert E.group_points_plan(1, 9, 64, 8196, threads=1024, target=2, nt=1, use_lds=1)["gx"] == 1
    assert E.group_points_plan(1, 9, 64, 8196, threads=1024, target=4, nt=0, use_lds=1) == dict(
        form="lds", T=1024, nt=0, gx=2, per_wg=8192, lds_bytes=2048, staged_vec=1, tail=1)
    assert E.group_points_plan(1, 9, 63, 2052, threads=256, target=1, nt=1, use_lds=1) == dict(
        form="lds", T=256, nt=1, gx=1, per_wg=3072, lds_bytes=8 * 63 * 4, staged_vec=0, tail=1)
    assert E.group_points_plan(2, 3, 64, 12, use_lds=0, threads=0, target=0, nt=1) == dict(
        form="direct_vec4", T=256, nt=0, gx=1, per_wg=1024, lds_bytes=0, staged_vec=0, tail=3)
    assert E.group_points_plan(2, 8, 64, 12, aligned=False, **T.DEFAULT_TUNE) == dict(
        form="direct_scalar", T=256, nt=0, gx=1, per_wg=256, lds_bytes=0, staged_vec=0, tail=0)
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)):
        with pytest.raises(ValueError):
            E.group_points_plan(*bad)
    # None: what the launcher currently uses -- the setter's value, else the environment's (read once per process)
    env = dict(use_lds=int(os.environ.get("PWCLO_GROUP_LDS", "1")), threads=int(os.environ.get("PWCLO_GP_THREADS", "0")),
               target=int(os.environ.get("PWCLO_GP_TARGET", "0")), nt=int(os.environ.get("PWCLO_GP_NT", "1")))
    shape = (1, 9, 64, 8196)
    assert E.group_points_plan(*shape) == E.group_points_plan(*shape, **env)
    try:
        E.group_points_tuning(use_lds=1, threads=512, target=4, nt=0)
        assert E.group_points_plan(*shape) == E.group_points_plan(*shape, use_lds=1, threads=512, target=4, nt=0)
        assert E.group_points_plan(*shape)["T"] == 512 and E.group_points_plan(*shape, threads=256)["T"] == 256
        E.group_points_tuning(use_lds=0)                      # every call sets all four: the other three are back
        assert E.group_points_plan(*shape) == E.group_points_plan(*shape, **dict(env, use_lds=0))
        assert E.group_points_plan(*shape)["form"] == "direct_vec4"
    finally:
        E.group_points_tuning()
    assert E.group_points_plan(*shape) == E.group_points_plan(*shape, **env)


@pytest.mark.parametrize("case", T.GROUP_CASES, ids=T.case_id)
def test_row_selects_the_form_it_names(E, case):
    P = case.s * case.k
    plan = T.plan_of(E, case)
    assert T.group_form(plan, P) == case.want, plan
    assert T.short_last_workgroup(plan, P) == case.opts.get("short_wg", False), plan
    assert plan["gx"] == case.opts.get("gx", plan["gx"]), plan
    # the staged rows on the stated side of 64 and 128 KiB (rows that state nothing are small)
    assert T.side(case.c, case.n) == case.opts.get("side", "<64K"), T.lds_need(case.c, case.n)
    if plan["form"] == "lds":
        assert plan["lds_bytes"] == T.lds_need(case.c, case.n) <= 128 * T.KIB
        assert plan["staged_vec"] == int(case.n % 4 == 0)
        lens = T.workgroup_lengths(plan, P)
        step = 4 * plan["T"]
        if case.want[4] == "several_short":
            assert any(L > step and 0 < L % step < step for L in lens), lens
        if case.want[4] == "one":
            assert max(lens) <= step
    else:
        assert plan["lds_bytes"] == 0
    assert plan["tail"] == case.c % 8
    # what makes the source-identity fill exact, and the index list hold what it must
    assert case.b * case.c * case.n < 2 ** 24 and case.s >= 3
    _, idx = T.group_inputs(case, "identity")
    flat = idx.reshape(case.b, P)
    assert idx.dtype == np.int32 and 0 <= idx.min() and idx.max() < case.n
    assert (flat[:, 0] == case.n - 1).all() and (flat[:, -1] == 0).all()
    assert (idx[:, case.s // 2] == idx[:, case.s // 2, :1]).all()


# ---- every form the dispatch can produce ----------------------------------------------------------------------------------
ALL_FORMS = set(itertools.product(("direct_scalar", "direct_vec4", "lds"), (1024, 512, 256), (1, 0), (1, 0), T.PASSES,
                                  (False, True)))
# what the code cannot produce: (which combinations, the line of csrc/group_points.hip that excludes them)
EXCLUDED = [
    ("a direct kernel with a workgroup other than 256 threads", lambda f: f[0] != "lds" and f[1] != 256,
     "dim3(GP_THREADS), 0, current_stream(), c, n, P, points, idx, out, out_bstride);"),
    ("the scalar kernel with the NT switch or staged rows", lambda f: f[0] == "direct_scalar" and (f[2] or f[3]),
     "return {PWCLO_GROUP_DIRECT_SCALAR, GP_THREADS, 0, ceil_div(P, GP_THREADS), GP_THREADS, 0, 0, c % GP_CH_PER_BLOCK};"),
    ("the direct 16-byte kernel with the NT switch or staged rows", lambda f: f[0] == "direct_vec4" and (f[2] or f[3]),
     "if (vec) return {PWCLO_GROUP_DIRECT_VEC4, GP_THREADS, 0, ceil_div(P / 4, GP_THREADS), GP_THREADS * 4, 0, 0, c % GP_CH_PER_BLOCK};"),
    ("a direct kernel with more than one pass: a thread handles one position (group) and returns",
     lambda f: f[0] != "lds" and f[4] != "one", "if (p >= P) return;"),
]

B_ = (1, 2)
C_ = (3, 8, 9)
N_ = (1, 3, 63, 64, 2044, 2048, 2052, 4096, 4097, 10922, 10923, 20000)
P_ = (1, 3, 4, 12, 255, 256, 257, 1024, 1028, 4096, 4100, 8192, 8196, 16388, T.THRESHOLD_P)
THREADS_ = (0, 256, 512, 100)
TARGET_ = (0, 1, 4)


@pytest.fixture(scope="module")
def reachable(E):
    forms = set()
    for b, c, n, p, al, lds, th, tg, nt in itertools.product(B_, C_, N_, P_, (0, 1), (0, 1), THREADS_, TARGET_, (0, 1)):
        plan = E.group_points_plan(b, c, n, p, aligned=al, use_lds=lds, threads=th, target=tg, nt=nt)
        forms.add(T.group_form(plan, p))
        key = (b, c, n, p, al, lds, th, tg, nt, plan)
        # what the kernels rely on
        if plan["form"] == "lds":
            step = 4 * plan["T"]
            assert plan["T"] in (1024, 512, 256) and p % 4 == 0 and al and lds, key
            assert plan["per_wg"] % step == 0 and plan["gx"] * plan["per_wg"] >= p > (plan["gx"] - 1) * plan["per_wg"], key
            assert plan["lds_bytes"] == T.lds_need(c, n) <= 128 * T.KIB and plan["nt"] == nt, key
        elif plan["form"] == "direct_vec4":
            assert p % 4 == 0 and al and (not lds or T.lds_need(c, n) > 128 * T.KIB), key
            assert plan["gx"] * 1024 >= p > (plan["gx"] - 1) * 1024, key
        else:
            assert (p % 4 != 0 or not al) and plan["gx"] * 256 >= p > (plan["gx"] - 1) * 256, key
    return forms


def test_case_table_wants_every_form_the_dispatch_can_produce(reachable):
    with open(SOURCE) as fh:
        source = fh.read()
    excluded = {}
    for what, pred, line in EXCLUDED:
        assert line in source, ("the excluding line is gone from group_points.hip", what)
        hit = {f for f in ALL_FORMS if pred(f)}
        assert hit, what
        for f in hit:
            excluded.setdefault(f, line)
    possible = ALL_FORMS - set(excluded)
    assert len(possible) == 72 + 4                  # every LDS combination; two tails of each direct kernel
    assert reachable == possible, (sorted(possible - reachable), sorted(reachable - possible))
    wanted = {c.want for c in T.GROUP_CASES}
    assert wanted == possible, ("not wanted by any row", sorted(possible - wanted), "cannot be", sorted(wanted - possible))
    # per T: both stagings, a narrow last slice, one pass, a short last pass and a short last workgroup; all six <T, NT> with
    # their dynamic LDS limit raised
    for Tn in (1024, 512, 256):
        rows = [c for c in T.GROUP_CASES if c.want[0] == "lds" and c.want[1] == Tn]
        assert {c.want[3] for c in rows} == {0, 1} and {c.want[4] for c in rows} == set(T.PASSES)
        assert {c.want[3] for c in rows if c.opts.get("short_wg")} == {0, 1}
        assert any(c.want[5] and c.want[4] == "several_short" and c.want[3] == st for c in rows for st in (0, 1))
        assert {c.want[2] for c in rows if T.lds_need(c.c, c.n) > 64 * T.KIB} == {0, 1}
    # direct scalar: c in {1, 7, 8, 9}, P below, at and one above 256; direct vec4: by size and by the switch
    scalar = [c for c in T.GROUP_CASES if c.want[0] == "direct_scalar"]
    assert {(c.c, c.s * c.k) for c in scalar} >= set(itertools.product((1, 7, 8, 9), (255, 256, 257)))
    assert all((c.s * c.k) % 4 != 0 or c.opts.get("misalign") for c in scalar)
    vec4 = [c for c in T.GROUP_CASES if c.want[0] == "direct_vec4"]
    assert {c.c for c in vec4 if c.tune["use_lds"] == 0} >= {8, 3, 9} and {c.c for c in vec4 if c.tune["use_lds"]} >= {8, 3, 9}
    assert any(c.s * c.k > 1024 for c in vec4)


def test_case_table_holds_both_sides_of_every_size_threshold(E):
    default = [c for c in T.GROUP_CASES if c.tune == T.DEFAULT_TUNE]
    # 128 KiB: LDS at n, the direct 16-byte kernel at n + 1, with c >= 8 and with c = 3
    for cmin, n in T.SIZE_THRESHOLDS:
        rows = [c for c in default if (c.c >= 8 if cmin == 8 else c.c == cmin)]
        assert any(c.n == n and c.want[0] == "lds" for c in rows) and any(c.n == n + 1 and c.want[0] == "direct_vec4" for c in rows)
        assert T.lds_need(cmin, n) <= 128 * T.KIB < T.lds_need(cmin, n + 1)
    # 64 KiB: the workgroup target flips from 512 to 256 between 2044 and 2048, the attribute is needed from 2052 on
    for n, side_ in zip(T.LDS_64K_ROWS, ("<64K", "=64K", ">64K")):
        assert any(c.n == n and c.c >= 8 and c.opts.get("side") == side_ for c in default), n
    lo, hi = [next(c for c in T.GROUP_CASES if c.n == n and c.s * c.k == T.THRESHOLD_P) for n in T.LDS_64K_ROWS[:2]]
    assert T.plan_of(E, lo) == T.plan_of(E, lo, target=512) != T.plan_of(E, lo, target=256)
    assert T.plan_of(E, hi) == T.plan_of(E, hi, target=256) != T.plan_of(E, hi, target=512)
    assert T.plan_of(E, lo)["gx"] == 257 and T.plan_of(E, hi)["gx"] == 129
    # the network's level-0 call
    assert any((c.c, c.n) == (3, 8192) and c.want[0] == "lds" and c.want[1] == 1024 for c in default)


def _group_shapes():
    with open(os.path.join(ROOT, "tests", "test_gpu_ops.py")) as fh:
        tree = ast.parse(fh.read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == "GROUP_SHAPES":
            return ast.literal_eval(node.value)
    raise AssertionError("GROUP_SHAPES not found in tests/test_gpu_ops.py")


def test_default_settings_select_the_launch_they_always_did(E):
    shapes = _group_shapes()
    assert len(shapes) >= 8
    for b, c, n, s, k in shapes:
        plan = E.group_points_plan(b, c, n, s * k, **T.DEFAULT_TUNE)
        assert launch_of(plan) == legacy_launch(b, c, n, s * k), (b, c, n, s, k, plan)
        if plan["form"] == "lds":
            tgt = 512 if plan["lds_bytes"] < 64 * T.KIB else 256
            assert plan["T"] == 1024 and plan["nt"] == 1
            assert plan == E.group_points_plan(b, c, n, s * k, use_lds=1, threads=1024, target=tgt, nt=1)
    assert {E.group_points_plan(b, c, n, s * k, **T.DEFAULT_TUNE)["form"] for b, c, n, s, k in shapes} == {"lds", "direct_scalar"}
    # and over the sweep's grid, with the thread counts the kernel exists for
    for b, c, n, p, al, lds, th, tg, nt in itertools.product(B_ + (32,), C_ + (64,), N_, P_, (0, 1), (0, 1), (0, 1024, 512, 256),
                                                             TARGET_, (0, 1)):
        plan = E.group_points_plan(b, c, n, p, aligned=al, use_lds=lds, threads=th, target=tg, nt=nt)
        assert launch_of(plan) == legacy_launch(b, c, n, p, al, lds, th, tg, nt), (b, c, n, p, al, lds, th, tg, nt, plan)


def test_other_thread_counts_are_sized_for_the_256_threads_that_run(E):
    for b, c, n, p in ((1, 9, 64, 8196), (2, 16, 2048, 32768), (1, 8, 2044, T.THRESHOLD_P), (2, 3, 8192, 2048), (1, 9, 63, 2052)):
        want = E.group_points_plan(b, c, n, p, use_lds=1, threads=256, target=0, nt=1)
        assert want["form"] == "lds" and want["T"] == 256
        for th in (1, 64, 100, 255, 257, 300, 768, 1000, 1023, 1025, 2048, 4096):
            assert E.group_points_plan(b, c, n, p, use_lds=1, threads=th, target=0, nt=1) == want, th
    # which is not what the value itself would have given
    assert legacy_launch(1, 9, 64, 8196, threads=100)[3:5] != launch_of(E.group_points_plan(1, 9, 64, 8196, threads=100, use_lds=1,
                                                                                            target=0, nt=1))[3:5]


# ---- the references catch what they must ----------------------------------------------------------------------------------
def _drop_sign(bits):
    return bits & np.int32(0x7FFFFFFF)


def _canonical_nan(bits):
    return np.where(np.isnan(bits.view(np.float32)), np.int32(0x7FC00000), bits)


def _differs(a, b):
    return bool((a != b).any())


def test_group_references_catch_the_planted_faults():
    caught = {"unwritten": 0, "shifted": 0, "sign": 0, "nan": 0}
    vec_rows = tail_rows = 0
    seen = set()
    for case in T.GROUP_CASES:
        if (case[:5]) in seen:                   # the same inputs under other settings
            continue
        seen.add(case[:5])
        P = case.s * case.k
        for kind in T.FILLS:
            bits, idx = T.group_inputs(case, kind)
            ref = T.ref_group(bits, idx)
            assert ref.shape == (case.b, case.c, case.s, case.k) and ref.dtype == np.int32
            assert not (ref == T.SENTINEL).any()
            want = T.ref_stack(ref, 2, 1)
            assert (want[:, :2] == T.SENTINEL).all() and (want[:, -1:] == T.SENTINEL).all()
            if P % 4 == 0:                        # the last 4 positions of a last pass left unwritten
                got = want.copy()
                got.reshape(case.b, -1, P)[:, 2:2 + case.c, P - 4:] = T.SENTINEL
                vec_rows += kind == "identity"
                caught["unwritten"] += kind == "identity" and _differs(got, want)
            if case.c % 8 and case.c > 1:         # the narrow last slice reads the channel after the one it should
                c0 = case.c - case.c % 8
                shifted = bits.copy()
                shifted[:, c0:] = bits[:, [(ch + 1) % case.c for ch in range(c0, case.c)]]
                tail_rows += kind == "identity"
                caught["shifted"] += kind == "identity" and _differs(T.ref_group(shifted, idx), ref)
            if kind == "identity":                # non-negative integers: blind to a lost sign or a changed NaN
                assert not _differs(_drop_sign(ref), ref) and not _differs(_canonical_nan(ref), ref)
            else:                                 # every index list reads a -0.0 and a negative NaN with a payload
                caught["sign"] += _differs(_drop_sign(ref), ref)
                caught["nan"] += _differs(_canonical_nan(ref), ref)
                assert (ref.reshape(case.b, case.c, P)[:, :, -1] == T.NEG_ZERO).all()
                assert (ref.reshape(case.b, case.c, P)[:, :, 0] == T.NEG_NAN_PAYLOAD).all()
    rows = len(seen)
    assert caught == {"unwritten": vec_rows, "shifted": tail_rows, "sign": rows, "nan": rows}, (caught, vec_rows, tail_rows, rows)
    assert vec_rows > 30 and tail_rows > 15


def test_gather_and_part_references_catch_the_planted_faults():
    assert {(c.m, c.c) for c in T.GATHER_CASES} == set(itertools.product((1, 255, 256, 257), (1, 8, 9)))
    for case in T.GATHER_CASES:
        for kind in T.FILLS:
            bits, idx = T.gather_inputs(case, kind)
            ref = T.ref_gather(bits, idx)
            assert ref.shape == (case.b, case.c, case.m) and 0 <= idx.min() and idx.max() < case.n
            if case.c > 1 and kind == "identity":
                assert _differs(T.ref_gather(np.roll(bits, -1, axis=1), idx), ref)
            if kind == "bits" and case.m >= 2:
                assert _differs(_drop_sign(ref), ref) and _differs(_canonical_nan(ref), ref)
    # broadcast_centre: k in {1, 3, 4, 5, 32}, P % 4 in {0, 1, 2, 3}, rows off the 16-byte grid
    assert {c.k for c in T.BCAST_CASES} >= {1, 3, 4, 5, 32}
    assert {(c.s * c.k) % 4 for c in T.BCAST_CASES if c.s > 1} == {0, 1, 2, 3}
    for k in (1, 3, 5):
        kinds = {(c.s * c.k) % 4 for c in T.BCAST_CASES if c.k == k and c.s > 1}     # straddling with and without a tail
        assert 0 in kinds and len(kinds) >= 2
    assert any(c.s * c.k > 1024 for c in T.BCAST_CASES)
    for case in T.BCAST_CASES:
        P = case.s * case.k
        starts = {((bb * (case.c_off + case.c + 2) + case.c_off + ch) * P * 4) % 16 for bb in range(case.b) for ch in range(case.c)}
        if P % 2 and case.c_off % 2 and case.s > 1:
            assert starts == {0, 4, 8, 12}, (case, starts)          # the 16-byte path and the tail path in one launch
        for kind in T.FILLS:
            bits = T.bcast_inputs(case, kind)
            ref = T.ref_bcast(bits, case.k)
            assert (ref == bits[:, :, :, None]).all()
            if case.s > 1 and kind == "identity":                    # j = p / k off by one position at a centre boundary
                assert _differs(T.ref_bcast(bits, case.k, shift=1), ref)
                assert ((T.ref_bcast(bits, case.k, shift=1) != ref).reshape(case.b, case.c, -1).sum(2) == case.s - 1).all()
            if kind == "bits" and case.s >= 2:
                assert _differs(_drop_sign(ref), ref) and _differs(_canonical_nan(ref), ref)
    # geometry_encode / xyz_diff: k in {1, 3, 32}, s * k around 256
    assert {c.k for c in T.GEO_CASES} == {1, 3, 32} and {c.s * c.k for c in T.GEO_CASES} >= {255, 256, 257, 258, 288}
    tiny = np.float32(np.sqrt(np.float64(np.float32(1e-20))))
    for case in T.GEO_CASES:
        for kind in T.FILLS:
            centre, src, idx = T.geo_inputs(case, kind)
            ref = T.ref_geo_copies(centre, src, idx)
            assert ref.shape == (case.b, 6, case.s, case.k) and (idx[:, :, 0] == np.arange(case.s)).all()
            assert (ref[:, 0:3, :, 0] == ref[:, 3:6, :, 0]).all()     # every centre is its own first neighbour
            if case.s > 1 and kind == "identity":
                assert _differs(T.ref_geo_copies(centre, src, idx, shift=1), ref)
            if kind == "bits" and case.s > 1:
                assert _differs(_drop_sign(ref), ref) and _differs(_canonical_nan(ref), ref)
        centre, src, idx = T.geo_inputs(case, "real")
        full = T.ref_geo(centre, src, idx)
        f = full.view(np.float32)
        assert np.isfinite(f).all() and (full[:, :6] == T.ref_geo_copies(centre, src, idx)).all()
        assert (full[:, 6:9, :, 0] == 0).all() and (f[:, 9, :, 0] == tiny).all() and tiny == np.float32(1e-10)
        # against float64: differences are exact or rounded once, the norm within a few ulp
        q, p = f[:, 3:6].astype(np.float64), f[:, 0:3].astype(np.float64)
        assert ((q - p).astype(np.float32) == f[:, 6:9]).all()
        e64 = np.sqrt(((q - p).astype(np.float32).astype(np.float64) ** 2).sum(1) + 1e-20)
        assert (np.abs(f[:, 9] - e64) <= 4 * 2.0 ** -24 * e64).all()
        assert (T.ref_xyz_diff(centre, src, idx).view(np.int32) == full[:, 6:9]).all()


def test_interpolation_reference():
    assert {(c.n, c.c) for c in T.INTERP_CASES} == set(itertools.product((1, 255, 256, 257), (1, 8, 9)))
    for case in T.INTERP_CASES:
        pts, idx, w = T.interp_inputs(case)
        assert 0 <= idx.min() and idx.max() < case.m and np.isfinite(pts).all()
        assert (w[:, 0].sum(-1) == 1).all() and set(np.unique(w[:, 0])) == {0.0, 1.0}          # weights 0 and 1
        ref = T.ref_interp(pts, idx, w)
        assert ref.shape == (case.b, case.c, case.n) and ref.dtype == np.float32
        exact = (pts.astype(np.float64)[np.arange(case.b)[:, None, None, None], np.arange(case.c)[None, :, None, None],
                                        idx[:, None].astype(np.intp)] * w[:, None].astype(np.float64)).sum(-1)
        mag = np.abs(pts)[np.arange(case.b)[:, None, None, None], np.arange(case.c)[None, :, None, None],
                          idx[:, None].astype(np.intp)].astype(np.float64) @ np.ones(3)
        assert (np.abs(ref - exact) <= 4 * 2.0 ** -24 * mag).all()
        for j in range(0, case.n, 5):           # a weight of exactly 1: the source's own bits (a zero partner adds +-0)
            sel = (j // 5) % 3
            src = pts[np.arange(case.b)[:, None], np.arange(case.c)[None, :], idx[:, j, sel][:, None].astype(np.intp)]
            assert (ref[:, :, j].view(np.int32) == src.view(np.int32)).all()


# ---- the search rows ------------------------------------------------------------------------------------------------------
def test_search_tables_hold_their_edge_cases():
    from oracle import ops as O
    assert {(c.m, c.n) for c in T.THREE_NN_CASES} == set(itertools.product((1, 2, 3, 63, 64, 65, 129, 200), (1, 3, 4, 5)))
    for case in T.THREE_NN_CASES:
        unknown, known = T.three_nn_inputs(case)
        dist, idx = O.three_nn(torch.from_numpy(unknown), torch.from_numpy(known))
        dist, idx = dist.numpy(), idx.numpy()
        same_lane = list(range(T.NN_SAME_LANE, case.m, 64))[:3]
        if len(same_lane) >= 2:                   # exact duplicates at k, k + 64 (, k + 128): one lane's running list
            assert list(idx[0, 0, :len(same_lane)]) == same_lane and (dist[:, 0, :len(same_lane)] == 0).all()
        if case.n > 1 and case.m > T.NN_NEXT_LANE + 1:      # and at k, k + 1: two lanes, popped in index order
            assert list(idx[0, 1, :2]) == [T.NN_NEXT_LANE, T.NN_NEXT_LANE + 1] and (dist[:, 1, :2] == 0).all()
        if case.m < 3:                            # empty slots: +inf and index 0
            assert np.isinf(dist[:, :, case.m:]).all() and (idx[:, :, case.m:] == 0).all()
        if case.m >= 63 and case.n >= 3:          # ties are the rule on the lattice
            assert (dist[:, :, 0] == dist[:, :, 1]).any() or (dist[:, :, 1] == dist[:, :, 2]).any()
    assert {(c.n, c.nsample) for c in T.BALL_CASES} == set(itertools.product((1, 63, 64, 65, 200), (1, 5, 64, 70)))
    for case in T.BALL_CASES:
        q, xyz = T.ball_inputs(case)
        idx = O.ball_query(torch.from_numpy(q), torch.from_numpy(xyz), T.BALL_RADIUS, case.nsample).numpy()
        assert idx.shape == (2, case.m, case.nsample)
        assert (idx[0, 2] == 0).all()             # no hit at all: the row keeps the front-end's fill
        hits0 = [i for i in T.BALL_Q0_HITS if i < case.n]
        want0 = (hits0 + [hits0[0]] * case.nsample)[:case.nsample] if hits0 else [0] * case.nsample
        assert list(idx[0, 0]) == want0           # the on-the-sphere candidates 0, 5 and 70 are not among them
        d2 = ((xyz[0][list(i for i in T.BALL_Q0_ON_SPHERE if i < case.n)] - q[0, 0]) ** 2).sum(1)
        assert (d2 == np.float32(T.BALL_RADIUS) ** 2).all()
        if case.n == 200:
            assert list(idx[0, 1]) == ([130, 150] + [130] * case.nsample)[:case.nsample]
            if case.nsample == 5:                 # fills in the middle of the second step, which holds 11 hits
                assert list(idx[0, 0]) == [2, 10, 50, 64, 65]
            if case.nsample == 70:                # more than 64 slots to pad
                assert case.nsample - len(T.BALL_Q1_HITS) > 64 and case.nsample - len(hits0) < 64
        # cloud 1 on the lattice: candidates exactly on the sphere exist and are excluded
        d2l = ((xyz[1][None] - q[1][:, None]) ** 2).sum(2)
        if case.n >= 63:
            assert (d2l == 4.0).any()
        for j in range(case.m):
            inside = np.nonzero(d2l[j] < 4.0)[0]
            assert set(idx[1, j]) <= (set(inside) or {0})
