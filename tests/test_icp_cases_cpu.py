"""The case table of tests/icp_cases.py holds what its names say, shown on the NumPy model alone: a pass of
tests/test_gpu_icp_edges.py then means that the kernels took the branches the cases aim at."""
import numpy as np
import pytest

import icp_cases as cases
import icp_model as model


# ---- normals -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", cases.normals_cases(), ids=lambda c: c["name"])
def test_normals_cases_reach_their_edge(c):
    x, n, k = c["xyz"], c["n"], c["k"]
    assert x.shape == (n, 3) and x.dtype == np.float32
    nrm, val, gap = model.normals(x, k)
    x64 = x.astype(np.float64)
    if c["edge"] in ("planar", "origin"):
        assert (x64 == np.round(x64)).all() and np.abs(x64).max() < 64           # short integers: every product is exact
        assert np.ptp(x64 @ c["plane_int"]) == 0.0                               # one plane, in integers
        assert nrm.any(axis=1).all() and (1.0 - np.abs(nrm @ c["plane"]) <= 64.0 * model.EPS64 / gap).all()
        assert gap.min() > 0.01
        if c["edge"] == "origin":
            assert (x64 @ c["plane_int"] == 0.0).all()
            for i in (0, n // 2, n - 1):                                         # the device's own eigenvector: exactly +z
                idx, _ = model.knn(x[i:i + 1], x, k + 1)
                d = x64[idx[0, 1:]] - x64[i]
                cov = [(d[:, a] * d[:, b]).sum() for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
                assert model.eig3(cov)[1].tolist() == [0.0, 0.0, 1.0]
        else:
            assert (x64 @ c["plane_int"] > 0.0).all()                                # every normal is flipped
    elif c["edge"] in ("rank_below", "rank_above"):
        ratio = val[:, 1] / val[:, 2]
        print("%s: l_mid / l_max in [%.3g, %.3g]" % (c["name"], ratio.min(), ratio.max()))
        if c["edge"] == "rank_below":                                            # a factor 1.5 from the threshold, every point
            assert (ratio * 1.5 < model.RANK_EPS).all() and (ratio > 0.01 * model.RANK_EPS).all() and not nrm.any()
        else:
            assert (ratio > 1.5 * model.RANK_EPS).all() and (ratio < 100 * model.RANK_EPS).all() and nrm.any(axis=1).all()
            assert (gap > 0.0).all()
    elif c["edge"] == "big":
        assert np.abs(x64).min() > 4.9e3
        left_out = (gap < model.GAP_MIN).mean()
        print("%s: left out %.4f" % (c["name"], left_out))
        assert left_out <= model.GAP_CAP
        assert len(np.unique(x[:, 0])) < n or np.spacing(x[0, 0]) > 9e-4         # the grid of fp32 at 1e4 is ~1e-3
    else:
        assert c["edge"] == "nan"
        assert (gap < model.GAP_MIN).mean() <= model.GAP_CAP
        idx, _ = model.knn(x, x, k + 1)
        hit = cases.nan_rows(c, idx)
        assert hit[c["nan_point"]] and hit.sum() > 1 and (k == n - 1) == bool(hit.all())
        assert np.isnan(cases.nan_cloud(c)).any(axis=1).sum() == 1


def test_jacobi_restatement_agrees_with_eigh():
    r = np.random.default_rng(3)
    for _ in range(50):
        d = r.normal(size=(12, 3)) * r.uniform(0.01, 10.0, 3)
        cov = d.T @ d
        val, vec = model.eig3([cov[0, 0], cov[0, 1], cov[0, 2], cov[1, 1], cov[1, 2], cov[2, 2]])
        w, v = np.linalg.eigh(cov)
        assert np.abs(val - w).max() <= 64.0 * model.EPS64 * w[2]
        assert 1.0 - abs(vec @ v[:, 0]) <= 64.0 * model.EPS64 * w[2] / (w[1] - w[0])


# ---- queries -------------------------------------------------------------------------------------------------------------------

def test_query_shapes():
    shapes = cases.QUERY_SHAPES
    assert {n for _, _, n in shapes} == {1, 255, 256, 257} and {M for _, M, _ in shapes} == {1, 64}
    assert any(S * M == 192 for S, M, _ in shapes)
    for S, M, n in shapes:
        c = cases.queries_case(S, M, n)
        assert c["p"].shape == (S, n, 3) and c["A"].shape == (S, M, 4, 4) and c["active"].tolist()[0] == 1
        assert S == 1 or (0 in c["active"] and 1 in c["active"])


# ---- accumulate ----------------------------------------------------------------------------------------------------------------

def test_accumulate_table_holds_every_shape_and_edge():
    names = [c["name"] for c in cases.accumulate_cases()]
    assert len(set(names)) == len(names)
    for n in cases.ACC_N:
        for M in cases.ACC_M:
            assert "shape-n%d-M%d" % (n, M) in names
    assert cases.ACC_N == (1, 63, 64, 65, 255, 256, 257, 513) and cases.ACC_M == (1, 3, 64)
    for name in ("all-dead", "single-first", "single-last-n257", "wave-0", "wave-1", "wave-2", "wave-3", "idx-rejected",
                 "nan-first-slot", "dist-inf", "max-dist-zero", "r-equals-sigma", "sigma-below-clamp", "r-zero"):
        assert name in names


@pytest.mark.parametrize("c", cases.accumulate_cases(), ids=lambda c: c["name"])
def test_accumulate_cases_reach_their_edge(c):
    S, M, n = c["S"], c["M"], c["n"]
    assert S == 3 and c["q"].shape == (S, M, n, 3) and c["idx"].dtype == np.int32 and c["dist"].dtype == np.float32
    # nothing out of range, not finite or tied outside the middle stream
    for s in (0, 2):
        live = c["live"][s] != 0
        assert ((c["idx"][s] >= 0) & (c["idx"][s] < n)).all() and np.isfinite(c["dist"][s][live]).all()
    for aim, s in c["aims"].items():
        hit = cases.branches(c, s)[aim]
        print("%s: %s taken by %d of %d points of stream %d" % (c["name"], aim, hit.sum(), n, s))
        assert hit.any(), aim
        assert aim in c["all"] or not hit.all(), aim
        assert aim not in c["all"] or hit.all(), aim
    # the rows per workgroup add up to the stream's row, and the groups hold what the case says
    for s in range(S):
        rows, mag = cases.case_groups(c, s)
        whole, _ = model.accumulate(*[c[k][s] for k in cases.ACC_KEYS], c["sigma"], c["max_dist"])
        assert rows.shape == ((n + 255) // 256, 32) and np.abs(rows.sum(axis=0) - whole).max() <= 1e-12 * max(1.0, mag.sum(axis=0).max())
        assert rows[:, model.PAIRS].sum() == whole[model.PAIRS] == cases.branches(c, s)["used"].sum()
        assert np.isfinite(rows).all()
    b = cases.branches(c, 1)
    if "only" in c:                                       # one pair, where the name says
        assert np.flatnonzero(b["used"]).tolist() == [c["only"]]
        rows, _ = cases.case_groups(c, 1)
        assert rows[:, model.PAIRS].tolist() == [1.0 if g == c["only"] // 256 else 0.0 for g in range(len(rows))]
    if c["name"] == "idx-rejected":
        seen = set(c["idx"][1, 1][b["index"]].tolist())
        assert seen == {-1, n, cases.INT_MIN, cases.INT_MAX} and b["index"][256] and b["used"].sum() == 3
        assert (b["slot"][b["index"]] == 1).all() and c["live"][1, 1] == 1
    if c["name"] == "nan-first-slot":
        assert b["nan_first"][:20].all() and b["nan_first"][256] and not b["used"][:20].any()
        assert (b["slot"][20:40] == 0).all() and b["nan_later"][20:40].sum() > 10
    if c["name"] == "dist-inf":
        assert (b["slot"][:20] == 1).all() and not b["used"][20:40].any() and b["inf_all"][20:40].all()
    if c["name"] == "dist-inf-max-dist-inf":
        assert b["used"][20:40].sum() > 10 and (b["slot"][20:40] == 0).all()
    if c["name"] == "max-dist-zero":
        assert b["dist_eq_max"][:10].sum() >= 8 and b["dist_eq_max"][256] and b["dist_above"][10:20].all() and not b["used"][10:20].any()
        assert not cases.branches(c, 0)["used"].any()
    if c["name"] == "r-equals-sigma":
        r = b["r"][b["used"]]
        assert sorted(np.abs(r).view(np.int64).tolist()).count(np.float64(c["sigma"]).view(np.int64)) == 2
        assert (np.abs(r) < c["sigma"]).sum() == 1 and (np.abs(r) > c["sigma"]).sum() == 1
    if c["name"] == "sigma-below-clamp":
        assert b["clamp"].sum() == 4 and b["above_clamp"].sum() == 2 and (b["used"] & (np.abs(b["r"]) < c["sigma"])).sum() == 1
        assert c["sigma"] < model.HUBER_CLAMP
    if c["name"] == "r-zero":
        assert b["r_zero"].sum() == 2 and b["used"].sum() == 3
    if c["name"].startswith("shape-") and M >= 3:
        assert c["live"][1].tolist() == [1, 0] + [1] * (M - 2) and np.isnan(c["dist"][1, 1]).all()


# ---- solve -------------------------------------------------------------------------------------------------------------------------

def test_solve_cases_reach_their_edges():
    assert cases.SOLVE_S == (1, 31, 32, 33, 65) and cases.SOLVE_G == (1, 2, 64)
    seen = {}
    for setting in cases.SOLVE_SETTINGS:
        for S in cases.SOLVE_S:
            for G in cases.SOLVE_G:
                c = cases.solve_case(setting, S, G)
                assert c["partial"].shape == (S, G, 32)
                for s in range(S):
                    w = cases.solve_expected(c, s)
                    seen.setdefault((setting, c["kinds"][s]), set()).add((w["status"], w["moved"]))
                    kind, row = c["kinds"][s], c["rows"][s]
                    if kind in cases.NAN_AT:
                        assert np.isnan(row[cases.NAN_AT[kind]]) and np.isnan(row).sum() == 1
                    else:
                        assert np.isfinite(row).all()
                    if kind in cases.EXACT_KINDS:
                        assert np.array_equal(row, cases._rows(kind))
                    if kind == "pairs_eq_min":
                        assert row[model.PAIRS] == c["min_pairs"] == 64
                    if kind == "pairs_below":
                        assert row[model.PAIRS] == 63
                    if setting in ("threshold", "above") and w["moved"] and w["status"] != model.BAD_PIVOT:
                        nd = np.linalg.norm(w["delta"])
                        if kind == "step_345":                                  # exact: no rounding anywhere
                            assert np.array_equal(w["delta"], cases.STEP_345) and nd == cases.T345 == 5 * 2.0 ** -10
                        else:
                            assert abs(nd - c["threshold"]) > 1e-6 * c["threshold"]
                    if kind == "near_pi" and w["moved"]:
                        assert abs(np.linalg.norm(w["delta"][:3]) - np.pi) < 1e-6
                    if kind == "zero_g" and c["it"] == 0:
                        assert not w["delta"].any() and np.abs(w["T"] - c["T_clean"][s]).max() <= 1e-15
    one = lambda key: seen[key]
    assert one(("first", "good")) == {(0, True)} and one(("first", "pairs_eq_min")) == {(0, True)}
    assert one(("first", "pairs_below")) == {(model.FEW_PAIRS, True)}
    for kind in ("nan_H", "nan_g", "nan_sw"):
        assert one(("first", kind)) == {(model.BAD_PIVOT, True)}, kind
    assert one(("first", "zero_g")) == {(model.CONVERGED, True)} and one(("zero", "zero_g")) == {(0, True)}
    assert one(("threshold", "step_345")) == {(0, True)} and one(("above", "step_345")) == {(model.CONVERGED, True)}
    assert one(("threshold", "one_pair")) == {(model.BAD_PIVOT, True)} and one(("zero", "one_pair")) == {(0, True)}
    # the general single pair: one pair, a Jacobian with every entry away from zero, a system of condition ~1e7, and a
    # bound that follows from that condition and stays far below the step itself
    row = cases._rows("one_pair_general")
    tol = cases.solve_tolerance("one_pair_general", row, 1e-6)
    diag = np.array([row[model.H0 + e] for e, (a, b) in enumerate(model.UPPER) if a == b]) / row[model.SW]
    assert row[model.PAIRS] == 1.0 and (diag > 1e-3).all() and one(("zero", "one_pair_general")) == {(0, True)}
    assert 1e6 < (diag.sum() + 1e-6) / 1e-6 < 1e8 and 1e-10 < tol < 1e-6 and cases.solve_tolerance("good", row, 1e-6) == 1e-10
    H, _ = model.system(row, 0.0)
    assert np.linalg.matrix_rank(H, tol=1e-9) == 1
    g = row[model.G0:model.G0 + 6] / row[model.SW]
    exact = -g / (diag.sum() + 1e-6)                                 # (J J^T + d I)^-1 J = J / (|J|^2 + d)
    mine = model.solve(row, np.eye(4), 0, 0, 1e-6, 0.0, 1)["delta"]
    err = np.abs(mine - exact).max() / np.abs(exact).max()
    print("general single pair: the model's own error %.3g, bound %.3g" % (err, tol))
    assert err <= 0.5 * tol                                          # the reference's own share of the bound
    assert all(st == 0 for key, v in seen.items() if key[0] == "zero" for st, _ in v)              # threshold 0: never
    later = set().union(*[v for key, v in seen.items() if key[0] == "later"])
    assert {(1, False), (2, False), (4, False), (8, False)} <= later and any(m for _, m in later)
    for S in (33, 65):                                                           # idle and active on both sides of a chunk
        a = cases.solve_case("first", S, 2)["active"]
        assert a[31] != a[32] or a[30] != a[32]
        assert 0 in a[:32] and 1 in a[:32] and a[32] == 0 and (S == 33 or (0 in a[33:] and 1 in a[33:]))


# ---- maps --------------------------------------------------------------------------------------------------------------------------

def test_maps_follow_icp_model_map():
    """The bit-exact restatement moves as icp_model.Map does (its products in BLAS order differ by roundings only)."""
    S, M, n = 3, 4, 64
    mine = cases.Maps(S, M, n, 0)
    mine.begin([1] * S, [1] * S)
    theirs = [model.Map(M, n, 10) for _ in range(S)]
    for k in range(6):
        f = cases.frame(S, n, k)
        T = f["T"].copy()
        T[:, 3] = (0.0, 0.0, 0.0, 1.0)
        mine.push(f["T"], f)
        for s in range(S):
            theirs[s].push(f["cloud"][s], T[s], f["normals"][s])
            assert np.abs(mine.A[s] - theirs[s].A).max() <= 1e-13 and np.abs(mine.R[s] - theirs[s].R).max() <= 1e-13
            assert mine.live[s].tolist() == theirs[s].live.tolist() and mine.cursor[s] == theirs[s].cursor
            live = theirs[s].live != 0                                           # a slot never filled holds what it was planted with
            assert np.array_equal(mine.xyz[s][live], theirs[s].xyz[live]) and np.array_equal(mine.normals[s][live], theirs[s].normals[live])


def test_maps_words_and_clamp():
    S, M, n = 3, 4, 65
    a = cases.Maps(S, M, n, 1)
    a.live[:] = 1
    a.cursor[:] = (-1, M, 2)
    before = {k: v.copy() for k, v in a.state().items()}
    f = cases.frame(S, n, 0)
    a.push(f["T"], f, active=[1, 1, 0], insert=[1, 1, 1])
    assert a.cursor.tolist() == [1, 0, 2]                                        # slot 0 and slot M - 1; the idle stream stays
    assert np.array_equal(a.xyz[0, 0], f["cloud"][0]) and np.array_equal(a.xyz[1, M - 1], f["cloud"][1])
    assert np.array_equal(a.xyz[2], before["map_xyz"][2]) and np.array_equal(a.A[2].view(np.int64), before["A"][2].view(np.int64))
    assert np.array_equal(a.A[0, M // 2, 3].view(np.int64), before["A"][0, M // 2, 3].view(np.int64))       # row 3 stays
    b = cases.Maps(S, M, n, 1)
    b.live[:] = 1
    keep = b.xyz.copy()
    b.push(f["T"], f, insert=[0, 0, 0])                                          # the gate says no: re-based only
    assert np.array_equal(b.xyz, keep) and b.live.all() and not np.array_equal(b.A[:, 0, :3], cases.Maps(S, M, n, 1).A[:, 0, :3])
    assert len(cases.words(2)) == 64 and len(cases.words(3)) == 512 and len({w.tobytes() for w in cases.words(3)}) == 512
    for nn in cases.PUSH_N:
        assert cases.ws_blocks(nn) == (3 if nn == 64 else 4)
