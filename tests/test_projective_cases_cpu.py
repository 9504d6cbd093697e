"""The conditions of tests/projective_cases.py, checked on the model alone (tests/projective_model.py): every case reaches
the edge it names, and tells the model from the planted fault that the edge is about (``projective_model.planted``), so that
tests/test_gpu_projective_edges.py cannot pass by missing it.

The plane cases print the fp64 uncertainty of a normal -- the largest disagreement between the model's LU solve and the
adjugate formula of proj_normal on the same moments.  Measured: 7.5e-13 at most (planes d = 5 and d = 0.5, K = 3 and 5),
and 1.4e-11 at most over the rough occupancy images; both far below a quarter of 2^-24 = 1.5e-8."""
import numpy as np
import pytest

import icp_model as icp
import projective_cases as C
import projective_model as model

F = np.float32


def differs(run, fault):
    """The faulty model's answer on a case is not the true model's."""
    true = run()
    with model.planted(fault):
        wrong = run()
    return any(not np.array_equal(a, b, equal_nan=True) for a, b in zip(true, wrong))


# ---- vertex map ----------------------------------------------------------------------------------------------------------------

VERTEX = C.vertex_cases()


def run_vertex(c):
    out = []
    for s in range(c["points"].shape[0]):
        out += model.vertex_map(c["points"][s], c["im"], None if c["lengths"] is None else c["lengths"][s],
                                None if c["keep"] is None else c["keep"][s])
    return out


@pytest.mark.parametrize("c", VERTEX, ids=[c["edge"] for c in VERTEX])
def test_vertex_case_reaches_its_edge(c):
    im, W = c["im"], c["W"]
    rows = run_vertex(c)[1::2]
    for s, pts in enumerate(c["points"]):
        row, col, r, valid, margin = model.pixels(pts, im)
        for i in range(len(pts)):
            if (s, i) not in c["exact"]:
                assert margin[i] >= C.BAND, (s, i, margin[i])            # inf for a point without a range
        for (t, i), (y, x) in c["lands"].items():
            if t == s:
                assert valid[i] and (row[i], col[i]) == (y, x), (s, i)
        for (t, i) in c["refused"]:
            if t == s:
                assert not valid[i], (s, i)
    for (s, y, x), i in c["wins"].items():
        assert rows[s][y, x] == i, (s, y, x)
    for fault in c["faults"]:
        assert differs(lambda: run_vertex(c), fault), fault


@pytest.mark.parametrize("H, W", C.EXACT_SHAPES)
def test_exact_arguments_are_exact(H, W):
    """The fp32 coordinates are exactly H / 2 and 0, W / 4, W / 2, 3 W / 4, W: nothing is left to the last bit."""
    c = C.exact_arguments(H, W)
    k = model.coords(c["points"][0, :5], c["im"])
    assert k["row32"].tolist() == [H / 2.0] * 5
    assert k["col32"].tolist() == [W / 2.0, W / 4.0, 3.0 * W / 4.0, 0.0, float(W)]
    assert np.signbit(c["points"][0, 4, 1]) and not np.signbit(c["points"][0, 3, 1])         # -0 against +0 decides the seam
    if (H, W) == (5, 10):
        assert np.rint(F(2.5)) == 2 and np.rint(F(7.5)) == 8             # half to even, down and up
    if (H, W) == (7, 6):
        assert np.rint(F(3.5)) == 4 and np.rint(F(1.5)) == 2 and np.rint(F(4.5)) == 4


@pytest.mark.parametrize("d", C.MARGINS)
def test_rows_and_seam_lie_where_they_say(d):
    c = C.rows_and_seam(d)
    H, W = c["H"], c["W"]
    k = model.coords(c["points"][0], c["im"])
    want_row, want_col = [-d, -1 + d, H - 1 + d, H - d], [W - 1 + d, W - d]
    assert np.abs(k["row64"][:4] - want_row).max() < 1e-5 and np.abs(k["row32"][:4] - want_row).max() < 1e-4
    assert np.abs(k["col64"][4:6] - want_col).max() < 1e-5 and np.abs(k["col32"][4:6] - want_col).max() < 1e-4
    rr = np.rint(k["row32"])
    assert rr[0] == 0 and np.signbit(rr[0])                              # row 0 through -0.0
    assert rr[1] == -1 and rr[2] == H - 1 and rr[3] == H and np.rint(k["col32"][5]) == W


def test_no_range_rows_have_none():
    c = C.no_range(3)
    bad = c["points"][0, 1::2]
    with np.errstate(all="ignore"):
        r = C.range32(bad)
    assert (bad[:3] != 0).any(axis=1).tolist() == [False, True, True]    # the origin; two points that are not the origin
    assert r[:3].tolist() == [0.0, 0.0, 0.0] and bad[2, 0] == np.nextafter(F(0), F(1))
    assert np.isinf(r[3]) and np.isfinite(bad[3]).all()                  # the overflow happens in the squares
    assert np.isnan(r[4:7]).all() and np.isinf(r[7:13]).all()
    for a in range(3):
        assert np.isnan(bad[4 + a, a]) and bad[7 + a, a] == np.inf and bad[10 + a, a] == -np.inf
    assert np.isnan(C.no_range(4)["points"][0, :, 3]).all()


@pytest.mark.parametrize("boundary", (False, True))
def test_zbuffer_ties_are_ties(boundary):
    c = C.zbuffer_ties(boundary)
    pts, pairs = c["points"][0], c["pairs"]
    r = C.bits32(C.range32(pts))
    pix = model.pixels(pts, c["im"])
    for a, b in pairs:
        assert a < b and (pix[0][a], pix[1][a]) == (pix[0][b], pix[1][b]) and pix[3][a] and pix[3][b]
        assert (a // 256 != b // 256) == boundary                       # the two rows are in different workgroups
    (a, b) = pairs[0]; assert r[a] == r[b] and pts[a].tobytes() == pts[b].tobytes()
    (a, b) = pairs[1]; assert r[b] < r[a]
    (a, b) = pairs[2]; assert r[b] < r[a]
    (a, b) = pairs[3]; assert r[a] == r[b] + 1                           # one ulp, either way round
    (a, b) = pairs[4]; assert r[b] == r[a] + 1
    assert c["points"].shape[1] >= (258 if boundary else 1)


def test_lengths_keep_and_row_counts():
    a, b = C.lengths_case(0), C.lengths_case(1)
    R = a["points"].shape[1]
    assert a["lengths"].tolist() + b["lengths"].tolist() == [-3, 0, 1, R, R + 5, 2]
    k = C.keep_case()
    assert k["lengths"] is None and k["keep"].tolist() == [[1, 1, 1, 1], [0, 1, 1, 1], [0, 0, 0, 0]]
    rows = run_vertex(k)[1::2]
    assert rows[0][2, 6] == 0 and rows[1][2, 6] == 1 and (rows[2] == -1).all()
    assert C.row_counts(1)["points"].shape[1] == 1 and C.row_counts(257)["points"].shape[1] == 257


# ---- normal map ----------------------------------------------------------------------------------------------------------------

def decidable(vmap, k):
    """No window with an occupied centre has a determinant within a factor of 10 of the cut, by either formula."""
    m, Cm = model.moments(np.asarray(vmap, dtype=F), k)
    occupied = (vmap != 0).any(axis=-1)
    with np.errstate(all="ignore"):
        for det in (np.abs(np.linalg.det(Cm))[occupied], np.abs(C.adjugate_normal(m, Cm)[1])[occupied]):
            det = det[~np.isnan(det)]
            if not ((det >= 1e-5) | (det <= 1e-7)).all():
                return False
    return True


@pytest.mark.parametrize("k", (3, 5))
@pytest.mark.parametrize("H, W", C.NORMAL_SHAPES)
def test_occupancy_reaches_corners_and_seams(H, W, k, capsys):
    c = C.occupancy(H, W)
    v = c["vmap"]
    occupied = (v != 0).any(axis=-1)
    assert 0.6 < occupied.mean() <= 1.0 and (H * W <= 40 or occupied.mean() < 0.95)
    assert occupied[0, 0] and occupied[0, -1] and occupied[-1, 0] and occupied[-1, -1]
    assert decidable(v, k)
    n = model.normal_map(v, k)[0]
    nz = (n != 0).any(axis=-1)
    assert nz.any() == (W > 1 and H * W > 1)                             # W = 1: every point in one plane with the sensor
    for x in C.SEAMS_X:
        assert x >= W or nz[:, x].any()                                  # normals on both sides of every seam
    for y in C.SEAMS_Y:
        assert y >= H or W == 1 or nz[y].any()
    bound = C.HALF_ULP + C.solve_disagreement(v, k)
    with capsys.disabled():
        print("\n[projective cases] occupancy %dx%d k=%d: fp64 solve disagreement %.2e" % (H, W, k, bound - C.HALF_ULP))
    assert bound - C.HALF_ULP < C.HALF_ULP / 4
    for fault in C.normal_faults(H, W, k):                                           # far more than the bound, not a last bit
        with model.planted(fault):
            wrong = model.normal_map(v, k)[0]
        assert np.abs(wrong - n).max() > 1e4 * bound, fault


@pytest.mark.parametrize("k", (3, 5))
def test_planes_give_their_normal_and_straddle_the_cut(k, capsys):
    for which in ("far", "near"):
        c = C.plane(which)
        n, det = model.normal_map(c["vmap"], k)
        hit = c["hit"]
        assert hit.sum() > 60 and (~hit).sum() > 60
        assert np.array_equal((n != 0).any(axis=-1), hit)               # every hit pixel has a normal
        assert (np.abs(det[hit]) >= 10.0 * 1e-6).all() and decidable(c["vmap"], k)
        assert np.abs(n[hit] - c["n"]).max() < 1e-4                      # the plane's own normal (the points are fp32)
        dis = C.solve_disagreement(c["vmap"], k)
        with capsys.disabled():
            print("\n[projective cases] plane d=%g k=%d: fp64 solve disagreement %.2e" % (c["d"], k, dis))
        assert dis < C.HALF_ULP / 4
    c = C.plane("cut")
    n, det = model.normal_map(c["vmap"], k)
    assert (np.abs(det[c["hit"]]) <= 1e-6 / 10.0).all() and not n.any() and decidable(c["vmap"], k)


@pytest.mark.parametrize("k", (3, 5))
def test_lonely_pixels(k):
    c = C.lonely()
    v = c["vmap"]
    n, det = model.normal_map(v, k)
    assert decidable(v, k)
    y, x = c["empty"]
    h = k // 2
    window = (v[y - h:y + h + 1, x - h:x + h + 1] != 0).any(axis=-1)
    assert window.sum() == k * k - 1 and not window[h, h]
    assert abs(det[y, x]) > 1e-5 and not n[y, x].any()                  # only the empty centre makes it zero
    assert n[y, x + 1].any() and n[y - 1, x].any()
    for at in (c["alone"],) + c["pair"] + c["column"]:                  # one point, two points, three in a plane with
        assert v[at].any() and abs(det[at]) <= 1e-7 and not n[at].any()     # the sensor: singular moments
    counts = [int((v[max(y - h, 0):y + h + 1, max(x - h, 0):x + h + 1] != 0).any(axis=-1).sum()) for y, x in
              (c["alone"], c["pair"][0], c["column"][1], c["triple"][0])]
    assert counts == [1, 2, 3, 3]                                        # the centre and none, one, two neighbours
    for at in c["triple"]:
        assert abs(det[at]) >= 1e-5 and n[at].any()                      # three points span a plane: a normal


@pytest.mark.parametrize("k", (3, 5))
def test_nan_vertex_spoils_its_windows_only(k):
    c = C.nan_vertex()
    y, x = c["at"]
    h = k // 2
    with np.errstate(all="ignore"):
        n = model.normal_map(c["vmap"], k)[0]
    clean = model.normal_map(c["emptied"], k)[0]
    yy, xx = np.meshgrid(np.arange(c["H"]), np.arange(c["W"]), indexing="ij")
    inside = (np.abs(yy - y) <= h) & (np.abs(xx - x) <= h)
    assert not n[inside].any() and clean[inside & ((yy != y) | (xx != x))].any(axis=-1).all()
    assert np.array_equal(n[~inside], clean[~inside]) and clean[~inside].any(axis=-1).all()
    assert decidable(c["emptied"], k)


# ---- model build ---------------------------------------------------------------------------------------------------------------

BUILD = C.build_cases()


def run_build(c):
    out = []
    for s in range(c["live"].shape[0]):
        b = model.model_build(c["map_v"][s], c["map_n"][s], c["A"][s], c["live"][s], c["im"])
        out += [b["src"], b["v"], b["n"]]
    return out


@pytest.mark.parametrize("c", BUILD, ids=[c["edge"] for c in BUILD])
def test_build_case_reaches_its_edge(c):
    S, M = c["live"].shape
    HW = c["H"] * c["W"]
    for s in range(S):
        b = model.model_build(c["map_v"][s], c["map_n"][s], c["A"][s], c["live"][s], c["im"])
        assert (b["margin"][np.isfinite(b["margin"])] >= C.BAND).all()
        src = b["src"].reshape(M, HW)
        assert np.isfinite(b["v"]).all() and np.isfinite(b["n"]).all()
        for m in range(M):
            assert (src[m] >= 0).any() == bool(c["live"][s, m])
            for name, t in c.get("plants", {}).get((s, m), {}).items():
                pix = model.pixels(C._moved(c["map_v"][s, m].reshape(HW, 3)[list(t[1:])], c["A"][s, m]), c["im"])
                assert pix[3].all() and (pix[0] * c["W"] + pix[1] == t[0]).all()      # the planted sources meet at one pixel
                r = C.bits32(pix[2])
                if name == "tie":
                    assert r[0] == r[1] and t[1] < t[2] and src[m, t[0]] == t[1]
                elif name == "nearer":
                    assert r[0] == r[1] and r[2] < r[0] and t[1] < t[2] < t[3] and src[m, t[0]] == t[3]
                else:
                    assert r[0] > r[1] and t[1] < t[2] and src[m, t[0]] == t[2]
    if "plants" in c:
        assert sorted(c["plants"]) == [(0, 0), (1, 1)]
        assert c["identity"] == (c["A"] == np.eye(4)).all()
    if "gone" in c:
        src = run_build(c)[0].reshape(-1)
        assert not np.isin(src, c["gone"]).any() and src[2 * c["W"]] == -1
        pts = c["map_v"].reshape(-1, 3)[list(c["gone"])]
        k = model.coords(pts, c["im"])
        assert np.rint(k["row32"][0]) < 0 and np.rint(k["col32"][1]) == c["W"] and C.range32(pts).max() < 2.0
    for fault in c.get("faults", ()):
        assert differs(lambda: run_build(c), fault), fault


def test_slot_cases_name_their_slots():
    assert C.slots("M=1")["live"].tolist() == [[1], [1]]
    c = C.slots("M=64")
    assert c["live"].shape == (2, 64) and np.flatnonzero(c["live"][0]).tolist() == [0, 31, 63]
    assert np.isnan(c["A"][0, 1]).all() and c["map_v"][0, 1].any()       # a dead slot: valid images, a pose of NaNs
    assert not C.slots("all dead")["live"].any()


# ---- accumulate ----------------------------------------------------------------------------------------------------------------

ACC = C.accumulate_cases()


def run_acc(c):
    out = []
    for s in range(c["vmap"].shape[0]):
        row, mag, a = model.accumulate(c["vmap"][s], c["model_v"][s], c["model_n"][s], c["T"][s], c["im"], c["sigma"],
                                       c["max_dist"])
        out += [a["slot"], a["own_pixel"], row]
    return out


@pytest.mark.parametrize("c", ACC, ids=[c["edge"] for c in ACC])
def test_accumulate_case_reaches_its_edge(c):
    out = run_acc(c)
    for s in range(c["vmap"].shape[0]):
        a = model.associate(c["vmap"][s], c["model_v"][s], c["model_n"][s], c["T"][s], c["im"], c["max_dist"])
        assert (a["margin"] >= C.BAND).all()
        assert np.isfinite(out[3 * s + 2]).all()
    for (s, i), m in c["slot"].items():
        assert out[3 * s][i] == m, (s, i)
    for (s, i), p in c["pixel"].items():
        assert out[3 * s + 1][i] == p, (s, i)
    for fault in c["faults"]:
        assert differs(lambda: run_acc(c), fault), fault


def test_accumulate_distances_are_exact():
    """The planted distances are the fp32 numbers they are said to be: ties are ties, max_dist is met with equality."""
    def dist(c, i, m, s=0):
        a = model.associate(c["vmap"][s], c["model_v"][s][m:m + 1], c["model_n"][s][m:m + 1], c["T"][s], c["im"], 1e9)
        return a["dist"][i]
    c = C.slot_ties()
    assert dist(c, 3, 0) == dist(c, 3, 2) == dist(c, 7, 0) == dist(c, 7, 2) == F(0.25)
    assert dist(c, 12, 0) == F(0.25) and dist(c, 12, 2) == F(0.125)
    c = C.max_dist_edge("equal")
    assert [dist(c, i, 0) for i in (3, 7, 12)] == [0.5, 0.0, 0.25]
    assert F(C.MAX_DISTS["below"]) < F(0.5) and F(C.MAX_DISTS["below"]) == np.nextafter(F(0.5), F(0))
    c = C.refusals()
    assert dist(c, 3, 0) == F(0.125) and dist(c, 3, 1) == F(0.25) and not c["model_n"][0, 0].reshape(-1, 3)[3].any()
    assert np.isnan(dist(c, 7, 0)) and dist(c, 7, 1) == F(0.125)
    k = model.coords(c["vmap"][0].reshape(-1, 3)[[31, 25]], c["im"])
    assert np.rint(k["row32"][0]) < 0 and np.rint(k["col32"][1]) == c["W"]
    c = C.translated()
    assert c["moved_off"] >= 5 and (c["T"][0][:3, 3] == [0.5, 0.0, 0.0]).all()
    a = model.associate(c["vmap"][0], c["model_v"][0], c["model_n"][0], c["T"][0], c["im"], c["max_dist"])
    paired = a["slot"] >= 0
    assert (a["dist"][paired] == F(0.125)).sum() >= 20                   # where two sources meet, the later candidate stands
    assert (a["q32"][paired].astype(np.float64) == c["vmap"][0].reshape(-1, 3)[paired].astype(np.float64) + [0.5, 0, 0]).all()


@pytest.mark.parametrize("H, W", C.REDUCTION_SHAPES)
def test_reduction_shapes_fill_the_workgroups_they_name(H, W):
    c = C.reductions(H, W)
    out = run_acc(c)
    assert [int(out[3 * s + 2][icp.PAIRS]) for s in range(3)] == list(c["pairs"])
    assert H * W in (1, 255, 256, 257) and not out[8].any()
    assert (out[3] == 0).all() and np.array_equal(out[4], np.arange(H * W))     # stream 1: every pixel pairs with itself


# ---- map push ------------------------------------------------------------------------------------------------------------------

PUSH = C.push_cases()


def run_push(c):
    t = {k: c[k].copy() for k in ("map_v", "map_n", "A", "live", "cursor")}
    model.map_push(c["T"], c["vmap"], c["nmap"], **t)
    return [t[k] for k in ("map_v", "map_n", "A", "live", "cursor")]


@pytest.mark.parametrize("c", PUSH, ids=[c["edge"] for c in PUSH])
def test_push_case_reaches_its_edge(c):
    M = c["M"]
    map_v, map_n, A, live, cursor = run_push(c)
    for s, m in enumerate(c["target"]):
        assert m == min(max(int(c["cursor"][s]), 0), M - 1) and cursor[s] == (m + 1) % M
        assert map_v[s, m].tobytes() == c["vmap"][s].tobytes() and (A[s, m] == np.eye(4)).all() and live[s, m] == 1
        others = np.arange(M) != m
        assert map_v[s, others].tobytes() == c["map_v"][s, others].tobytes()
        dead = others & (c["live"][s] == 0)
        assert A[s, dead].tobytes() == c["A"][s, dead].tobytes()
        moved = others & (c["live"][s] != 0)
        assert M == 1 or moved.any() or dead.any()
    assert sorted(set(C.push(M, 0)["cursor"].tolist() + C.push(M, 1)["cursor"].tolist())) == sorted({-5, 0, M - 1, M, 99})
    assert differs(lambda: run_push(c), "no_cursor_clamp")
