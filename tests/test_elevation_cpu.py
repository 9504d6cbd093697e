"""The loop detector's translation search without a GPU: the fp32 model against a plain fp64
restatement, the signs of (k, a, b) on lattice clouds, the ``up="-y"`` permutation, the edge rows, the search rules, a table of
planted faults, the host refusals and tables, the launches of ``translation=None``, and the margins of the whole-chain scene."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elevation_cases as EC            # noqa: E402
import elevation_model as EM            # noqa: E402
import icp_model as IM                  # noqa: E402
import loop_closure_cases as C          # noqa: E402
import loop_closure_model as LM         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW = ["elevation_image_kernel_wrapper", "elevation_score_kernel_wrapper", "elevation_choose_kernel_wrapper"]


def test_model_agrees_with_the_fp64_restatement():
    """Points at cell centres and level middles are far from every edge, so only the binning's precision separates the two."""
    p = dict(EM.DEFAULTS, cells=32, window=4)
    cloud = EC.lattice(3, p, fill=0.4)
    for shift, k in ((0, 4), (7, 0), (52, 8)):
        theta = EM.angle(shift, k, EC.SECTORS, p["yaw_div"], p["yaw_half"])
        query = EC.seen_from(cloud, shift, k, 1, -2, p)
        rot = EM.tables(EC.SECTORS, p["yaw_div"], p["yaw_half"])[0][shift * 9 + k]
        a = EM.grid(query.astype(F), rot[0], rot[1], 32, 1.0, 0.25, EC.Z_OFFSET)
        b = EM.grid64(query, theta, 32, 1.0, 0.25, EC.Z_OFFSET)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[1] > 50


@pytest.mark.parametrize("up", ["z", "-y"])
def test_a_moved_lattice_gives_back_its_offset(up):
    """Pins the signs: the query's pose in the stored frame is [Rz(theta_k), (a c, b c, 0)], and the search reads back exactly
    (k, a, b) with every cell in full agreement; T1 then maps the query's points onto the stored ones."""
    for cell_size, (shift, k, a, b) in ((1.0, (7, 2, 3, -2)), (0.5, (52, 0, -4, 1)), (1.0, (0, 1, 0, 0)), (2.0, (33, 1, -1, -4))):
        p = dict(EC.SMALL, cells=32, window=4, cell_size=cell_size)
        stored = EC.lattice(shift + 1, p)
        query = EC.seen_from(stored, shift, k, a, b, p)
        if up == "-y":
            stored, query = C.to_camera(stored), C.to_camera(query)
        out = EM.search(stored.astype(F), query.astype(F), shift, EC.SECTORS, p, up=up)
        rec = out["record"]
        assert (rec["found"], rec["k"], rec["a"], rec["b"]) == (1, k, a, b), rec
        assert rec["A"] == p["tolerance"] * rec["occ_q"] and rec["occ_q"] == rec["occ_e"] == len(stored)
        T1 = out["T1"]
        assert np.abs(query @ T1[:3, :3].T + T1[:3, 3] - stored).max() <= 1e-9


def test_camera_frame_equals_the_permuted_cloud():
    p = dict(EC.SMALL)
    rows = np.concatenate([EC.edge_rows(p), C.random_cloud(3, 300, max_range=10.0)])
    lat = EC.lattice(2, p).astype(F)
    a = EM.search(lat, rows, 5, EC.SECTORS, p)
    b = EM.search(C.to_camera(lat).astype(F), C.to_camera(rows).astype(F), 5, EC.SECTORS, p, up="-y")
    for key in ("E", "Q", "occ_q", "A"):
        assert np.array_equal(a[key], b[key]), key
    assert a["record"] == b["record"] and a["record"]["A"] > 0


def test_edge_rows_lie_where_the_specification_puts_them():
    p = dict(EC.SMALL)
    G, c, zs = p["cells"], F(p["cell_size"]), F(p["z_step"])
    rows = EC.edge_rows(p)
    keep, i, j, q = EM.cells_of(rows, F(1), F(0), G, c, zs, EC.Z_OFFSET)
    x, y, z = rows[:, 0], rows[:, 1], rows[:, 2]
    finite = np.isfinite(rows).all(axis=1)
    assert (~finite).sum() == 9 and not keep[~finite].any()
    for axis, v, cell in ((0, x, i), (1, y, j)):
        other = (y if axis == 0 else x)
        mid = finite & (np.abs(other) < 7.0) & (z > 0)              # rows of this axis' groups
        for k in (-1, 0, 1, G // 2 - 1):                            # x / c on an integer: the cell starts there
            on = mid & (v == F(k) * c)
            assert on.any() and keep[on].all() and (cell[on] == k + G // 2).all()
            below = mid & (v == EC.down_(F(k) * c))
            assert below.any() and keep[below].all() and (cell[below] == k - 1 + G // 2).all()
        low, high = F(-G // 2) * c, F(G // 2) * c
        assert keep[mid & (v == low)].all() and (cell[mid & (v == low)] == 0).all() and (mid & (v == low)).any()
        assert (mid & (v == EC.down_(low))).any() and not keep[mid & (v == EC.down_(low))].any()     # outside by one ulp
        assert (mid & (v == high)).any() and not keep[mid & (v == high)].any()                       # the upper edge is open
        assert keep[mid & (v == EC.down_(high))].all() and (cell[mid & (v == EC.down_(high))] == G - 1).all()
    with np.errstate(all="ignore"):
        h = z + F(EC.Z_OFFSET)
    assert (h[finite] == 0).any() and not keep[finite & (h <= 0)].any()
    tiny = finite & (h > 0) & (h < zs) & (x == F(-2.5) * c)
    assert tiny.any() and keep[tiny].all() and (q[tiny] == 1).all()                                  # the first level above 0
    top = finite & (x == F(1.5) * c)
    with np.errstate(all="ignore"):
        lev = np.floor(h / zs)
    assert set(lev[top]) >= {251.0, 252.0, 253.0, 254.0, 255.0}
    assert (q[top & (lev == 253)] == 254).all() and (q[top & (lev >= 254)] == 255).all() and (q[top & (lev == 252)] == 253).all()
    inf = finite & (z > 1e30)
    assert np.isinf(lev[inf]).all() and keep[inf].all() and (q[inf] == 255).all()
    short = EM.grid(rows, F(1), F(0), G, c, zs, EC.Z_OFFSET, length=10)
    assert short[1] <= 10 and short[1] < EM.grid(rows, F(1), F(0), G, c, zs, EC.Z_OFFSET)[1]        # rows past the length
    assert EM.grid(rows, F(1), F(0), G, c, zs, EC.Z_OFFSET, length=-3)[1] == 0


def _case(name):
    return next(c for c in EC.rule_cases() if c["name"] == name)


def _model(case, **kw):
    return EM.search(case["stored"], case["query"], case["shift"], EC.SECTORS, case["p"], length=case["length"], **kw)


def test_search_rules_in_the_model():
    W = EC.SMALL["window"]
    rec = _model(_case("tie"))["record"]
    assert (rec["found"], rec["k"], rec["a"], rec["b"], rec["A"]) == (1, 0, -2, 0, 4)        # a = -2 and a = +2 tie: the lower
    rec = _model(_case("tie over yaw"))["record"]
    assert (rec["k"], rec["a"], rec["b"]) == (0, 0, 0)                   # a cell at the centre under every yaw: the lowest k
    for name in ("empty query", "empty stored"):
        out = _model(_case(name))
        assert out["record"]["found"] == 0 and out["record"]["A"] == 0 and not out["A"].any()
        assert (out["record"]["k"], out["record"]["a"], out["record"]["b"]) == (0, -W, -W)
        assert np.array_equal(out["T1"], LM.start_pose(0, EC.SECTORS))   # not found: T0 as it is
    at, below = _model(_case("acceptance at the bound"))["record"], _model(_case("acceptance one below"))["record"]
    assert (at["A"], at["found"], at["occ_q"], at["occ_e"]) == (8, 1, 4, 4) and (below["A"], below["found"]) == (7, 0)
    fewer = _model(_case("fewer query cells than stored"))["record"]
    assert (fewer["A"], fewer["occ_q"], fewer["occ_e"], fewer["found"]) == (4, 2, 4, 1)      # min, not max: 4 >= 0.5 * 4 * 2
    zero = _model(_case("window 0"))
    assert zero["A"].shape == (3, 1, 1) and (zero["record"]["a"], zero["record"]["b"], zero["record"]["found"]) == (0, 0, 1)
    one = _model(_case("one yaw"))
    assert one["A"].shape == (1, 7, 7) and (one["record"]["k"], one["record"]["a"], one["record"]["b"]) == (0, 1, 1)


def test_the_second_implementation_is_the_model():
    for case in EC.rule_cases():
        for up in ("z", "-y"):
            c = case if up == "z" else dict(case, stored=C.to_camera(case["stored"]).astype(F),
                                            query=C.to_camera(case["query"]).astype(F))
            assert EC.same(EC.variant(c, up=up), _model(c, up=up)), (case["name"], up)


@pytest.mark.parametrize("fault", EC.FAULTS)
def test_the_table_catches_a_planted_fault(fault):
    """Each mistake a kernel could make changes an image, a score, the record or the seed of at least one case."""
    caught = [case["name"] for case in EC.rule_cases() if not EC.same(EC.variant(case, fault=fault), _model(case))]
    assert caught, fault


# ---- host logic ---------------------------------------------------------------------------------------------------------------

def test_host_refusals():
    from pwclonet_pylidarslam_amd import loop_closure as L
    make = lambda **kw: L.ScanContextLoopDetector(1, 128, **kw)
    for t in (dict(cells=6), dict(cells=130), dict(cells=33), dict(cells=32.0), dict(cell_size=0.0), dict(cell_size=float("inf")),
              dict(cell_size=float("nan")), dict(cell_size=1e-60), dict(window=-1), dict(window=17), dict(yaw_div=0),
              dict(yaw_div=9), dict(yaw_half=-1), dict(yaw_half=9), dict(z_step=0.0), dict(z_step=-1.0), dict(tolerance=0),
              dict(tolerance=256), dict(min_agreement=-0.1), dict(min_agreement=1.5), dict(min_agreement=float("nan")),
              dict(levels=3), dict(window=True)):
        with pytest.raises(ValueError, match="ScanContextLoopDetector: translation="):
            make(translation=t)
    with pytest.raises(ValueError, match="translation= images the stored clouds"):
        make(translation=dict(), verify=None)
    det = make(translation=dict(cells=8, window=0))
    assert det.translation == dict(L.TRANSLATION_DEFAULTS, cells=8, window=0) and det.seed() is None
    assert make().translation is None and make().seed() is None
    assert L.TRANSLATION_DEFAULTS == EM.DEFAULTS
    base = make().map_bytes()
    assert make(translation=dict()).map_bytes() == base + 10 * (128 * 128 + 4) + 9 * 128 * 128 * 4 + 9 * 33 * 33 * 4 + 32 + 128


def test_tables_are_the_models():
    from pwclonet_pylidarslam_amd import loop_closure as L
    for sectors, d, Yh in ((60, 2, 4), (8, 1, 0), (64, 8, 8)):
        for up in ("z", "-y"):
            rot, pose = L.elevation_tables(sectors, d, Yh, up)
            mrot, mpose = EM.tables(sectors, d, Yh, up)
            assert rot.dtype == np.float32 and rot.shape == (sectors * (2 * Yh + 1), 2) and np.array_equal(rot, mrot)
            assert np.array_equal(pose, mpose)
            Y = 2 * Yh + 1
            for s in (0, 1, sectors - 1):                               # the middle candidate is Scan Context's own T0
                assert np.abs(pose[s * Y + Yh] - LM.start_pose(s, sectors, up)).max() <= 1e-15


def test_abi_symbols():
    from pwclonet_pylidarslam_amd import _lib, build
    with open(os.path.join(ROOT, "include", "pwclo_ops.h")) as f:
        header = f.read()
    lib = ctypes.CDLL(build.build())
    for name in NEW:
        m = re.search(r"void\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m is not None, "%s is not declared in include/pwclo_ops.h" % name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][0]), name
        assert hasattr(lib, name), name


class _Refiner:
    bufs = dict(status=None, pairs=None, cost=None)

    def __init__(self, log):
        self.log = log

    def register(self, cloud, T, active=None, restart=None):
        self.log.append(("register", cloud.data_ptr(), T.data_ptr()))
        return T


def _launches(monkeypatch, translation):
    """The argument lists one detection hands the library, on CPU tensors, with the library and the refiner stubbed."""
    from pwclonet_pylidarslam_amd import _lib, loop_closure as L
    log = []
    monkeypatch.setattr(_lib, "load", lambda: None)
    monkeypatch.setattr(_lib, "call", lambda name, device, *args: log.append((name,) + args))
    det = L.ScanContextLoopDetector(2, 64, max_keyframes=4, device="cpu", translation=translation)
    det._alloc()
    det._refiner = _Refiner(log)
    det._body(None)
    return det, log


def test_translation_none_launches_what_the_parent_launched(monkeypatch):
    """``translation=None`` adds no buffer and no launch, and every launch takes its buffers in the parent's order (the
    parent's argument lists, restated here); with the keyword the three launches sit between fetch and the registrations
    and the second registration starts from T1."""
    det, log = _launches(monkeypatch, None)
    b = det.bufs
    assert not [k for k in b if k.startswith("ei_") or k == "T1"]
    p = lambda k: b[k].data_ptr()
    assert [e[0] for e in log] == ["scan_context_build_kernel_wrapper", "loop_score_kernel_wrapper", "loop_select_kernel_wrapper",
                                   "loop_fetch_kernel_wrapper", "register", "register", "loop_accept_kernel_wrapper",
                                   "loop_insert_kernel_wrapper"]
    assert log[0][1:] == (2, 64, 20, 60, 0, 2.0, p("cloud"), p("lengths"), p("ring_b"), p("sector_d"), p("D"), p("Dn"), p("qmask"),
                          p("active"), p("restart"), p("count"), p("nlog"), p("epoch"))
    assert log[1][1:] == (2, 20, 60, 4, p("Dn"), p("qmask"), p("db_desc"), p("db_mask"), p("db_frame"), p("count"), p("active"),
                          p("frame_id"), 200, 0, 0, 0.0, p("scores"), p("shifts"))
    assert log[2][1:] == (2, 60, 4, 1, 0.2, p("scores"), p("shifts"), p("db_frame"), p("count"), p("active"), p("frame_id"),
                          p("T0_table"), p("match"), p("match_score"), p("found"), p("T0"), p("slot"), p("overflow"))
    assert log[3][1:] == (2, 64, 4, p("found"), p("match"), p("db_cloud"), p("staging"))
    assert log[4] == ("register", p("staging"), p("eye")) and log[5] == ("register", p("cloud"), p("T0"))
    assert log[6][1:] == (2, 64, 256, p("found"), p("match"), p("match_score"), p("frame_id"), p("T0"), 0, 0, 0, 0.3, 0.25,
                          p("log_i"), p("log_T"), p("log_c"), p("nlog"), p("log_overflow"), p("accepted"))
    assert log[7][1:] == (2, 64, 20, 60, 4, p("slot"), p("frame_id"), p("Dn"), p("qmask"), p("cloud"), p("db_desc"), p("db_mask"),
                          p("db_frame"), p("db_cloud"), p("count"))
    det2, log2 = _launches(monkeypatch, dict(cells=16, window=3, yaw_half=1))
    q = lambda k: det2.bufs[k].data_ptr()
    names = [e[0] for e in log2]
    assert names[3:9] == ["loop_fetch_kernel_wrapper", "elevation_image_kernel_wrapper", "elevation_score_kernel_wrapper",
                          "elevation_choose_kernel_wrapper", "register", "register"] and len(names) == 11
    assert log2[7] == ("register", q("staging"), q("eye")) and log2[8] == ("register", q("cloud"), q("T1"))
    assert log2[4][1:10] == (2, 64, 60, 16, 3, 0, 2.0, 1.0, 0.25) and log2[5][1:6] == (2, 16, 3, 3, 4)
    assert log2[6][1:9] == (2, 60, 3, 3, 4, 0, 0.5, 1.0)
    for old, new in zip(log[:4] + log[6:], log2[:4] + log2[9:]):         # the parent's launches keep their scalar arguments
        assert old[0] == new[0] and [x for x in old[1:] if isinstance(x, float)] == [x for x in new[1:] if isinstance(x, float)]


def test_the_keyword_reaches_the_detector_through_both_front_doors():
    from pwclonet_pylidarslam_amd.loop_closure import ScanContextLoopClosure
    from pwclonet_pylidarslam_amd.odometry import StreamingOdometry
    lc = ScanContextLoopClosure(128, device="cpu", translation=dict(cells=32, window=8))
    assert lc.detector().translation["cells"] == 32 and lc.detector().translation["yaw_half"] == 4
    with pytest.raises(ValueError, match="translation="):
        ScanContextLoopClosure(128, device="cpu", translation=dict(cells=7))
    so = StreamingOdometry(None, streams=1, backend=dict(), loop=dict(translation=dict(window=4)))
    assert so._loop_cfg["translation"] == dict(window=4)


# ---- the whole chain on the model ----------------------------------------------------------------------------------------------

def _verify(stored, query, start):
    """``icp_model.register`` against the stored cloud -> (T, status, pairs, cost) as the refiner records them: pairs and cost
    of the last iteration that ran."""
    mp = IM.Map(1, len(stored), 10)
    mp.push(stored, np.eye(4))
    T, status, steps = IM.register(mp, query, start, push=False, **EC.OFFSET_VERIFY)
    state, last = 0, None
    for s in steps:
        if state == 0:
            last = s["row"]
        state = s["status"]
    return T, status, int(last[IM.PAIRS]), float(last[IM.COST])


def _error(T, truth):
    d = np.linalg.inv(truth) @ T
    return float(np.linalg.norm(d[:3, 3])), float(np.arccos(np.clip((np.trace(d[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))


def test_offset_revisit_scene_has_margins():
    """What tests/test_gpu_elevation_stream.py asserts on the device, decided here by the model chain with margins.  The
    return passes 2.01 m beside the start (2 x the verifying ``max_dist`` of 1 m).  Scan Context: only the last frame is a
    match (0.153 against the threshold 0.2; the others 0.36 and more), 4 x the fp32 model's error clear of it.  (a) From T0
    the refiner pairs 75 % of the points at a mean cost of 0.100, slides along the floor and the walls and comes to rest
    2.46 m from the truth: refused by ``min_fitness`` 0.9 and ``max_mean_cost`` 0.06 (the defaults 0.3 and sigma^2 would log
    this false closure).  (b) The translation search finds (k, a, b) = (5, 0, -2) with A = 458 against the bound 371.2; from
    T1 the refiner pairs 98.8 % at 0.027 and rests 1.003 x as far from the truth as when it starts from the truth."""
    c = EC.offset_revisit()
    path, frames = c["path"], c["frames"][:, 0]
    K, n = len(path), EC.OFFSET_N
    p = dict(EM.DEFAULTS, **EC.OFFSET_TRANSLATION)
    desc = [LM.descriptor(f) for f in frames]
    matches = []
    for j in range(EC.OFFSET_MIN_ID, K):
        ids = np.arange(0, j - EC.OFFSET_MIN_ID + 1)
        ok = LM.eligible(ids, j, EC.OFFSET_MIN_ID, c["positions"], EC.OFFSET_MAX_DISTANCE)
        d2 = ((c["positions"][ids] - c["positions"][j]) ** 2).sum(axis=1)
        assert np.abs(d2 - EC.OFFSET_MAX_DISTANCE ** 2).min() > 1e-6              # no place sits on the gate
        if not ok.any():
            continue
        args = (desc[j][1], desc[j][2], [desc[i][1] for i in ids[ok]], [desc[i][2] for i in ids[ok]])
        d64, d32 = LM.distances64(*args), LM.distances(*args)
        err = float(np.abs(d32.astype(np.float64) - d64)[np.isfinite(d64)].max())
        assert abs(d64.min() - EC.OFFSET_THRESHOLD) > max(4 * err, 0.04), (j, d64.min())
        if d64.min() < EC.OFFSET_THRESHOLD:
            e = int(d64.min(axis=1).argmin())
            row, best = np.sort(d64[e]), d64.min(axis=1)
            assert row[1] - row[0] > 4 * err and (len(best) == 1 or np.delete(best, e).min() - best[e] > 4 * err)
            matches.append((j, int(ids[ok][e]), int(d64[e].argmin())))
    assert matches == [(K - 1, 0, 57)], matches
    j, i, shift = matches[0]
    truth = np.linalg.inv(path[i]) @ path[j]
    assert np.linalg.norm(truth[:3, 3]) >= 1.5 * EC.OFFSET_VERIFY["max_dist"] + 0.5
    fit, cost = EC.OFFSET_ACCEPT["min_fitness"], EC.OFFSET_ACCEPT["max_mean_cost"]
    # (a) from T0
    T, status, pairs, total = _verify(frames[i], frames[j], LM.start_pose(shift, EC.SECTORS))
    print("from T0: status", status, "fitness", pairs / n, "mean cost", total / pairs, "error", _error(T, truth))
    assert pairs / n < fit - 0.1 and total / pairs > 1.5 * cost and _error(T, truth)[0] > 1.0
    # (b) from T1
    out = EM.search(frames[i], frames[j], shift, EC.SECTORS, p)
    rec = out["record"]
    bound = p["min_agreement"] * p["tolerance"] * min(rec["occ_q"], rec["occ_e"])
    print("record", rec, "bound", bound)
    assert rec["found"] == 1 and (rec["k"], rec["a"], rec["b"]) == (5, 0, -2) and rec["A"] > 1.15 * bound
    runner = np.sort(out["A"].reshape(-1))[-2]
    assert rec["A"] > runner                                                      # no tie decides the seed
    assert _error(out["T1"], truth)[0] < 0.5 * EC.OFFSET_VERIFY["max_dist"]
    T, status, pairs, total = _verify(frames[i], frames[j], out["T1"])
    yard = _error(_verify(frames[i], frames[j], truth)[0], truth)
    got = _error(T, truth)
    print("from T1: status", status, "fitness", pairs / n, "mean cost", total / pairs, "error", got, "fixed point", yard,
          "ratios", got[0] / yard[0], got[1] / yard[1])
    assert (status & (IM.FEW_PAIRS | IM.BAD_PIVOT)) == 0 and pairs / n > fit + 0.05 and total / pairs < 0.6 * cost
    assert got[0] <= 2 * yard[0] and got[1] <= 2 * yard[1]                        # the device test allows 4 x
