"""Every kernel of the loop detector alone (csrc/loop_closure.hip, csrc/elevation.hip) on the named edge
cases of tests/loop_closure_edge_cases.py, which tests/test_loop_closure_edges_cpu.py proves to take the branches their names
say, against the NumPy model (tests/loop_closure_model.py, tests/elevation_model.py).  One launch per check, through the
detector's own methods on ``det.bufs`` or through ``_lib.call`` on the test's tensors; no whole detection but the one test of
raw mode with ``loop=``.

Every tensor a kernel may write is a view into a larger allocation with the guard bands of tests/test_gpu_icp_edges.py on
either side, checked after the call, and starts as a NaN of a fixed bit pattern (-7 for integers), so "written" and "left
alone" are told apart to the bit.  Every comparison is to the bit: floats as integers, poses as bytes, lists as sets."""
import numpy as np
import pytest
import torch

import elevation_cases as ELC
import elevation_model as EM
import loop_closure_edge_cases as EC
import loop_closure_model as M
import loop_closure_second as K
from pwclonet_pylidarslam_amd import _lib
from pwclonet_pylidarslam_amd import loop_closure as L
from test_gpu_icp_edges import Guards, _p, _raw

pytestmark = pytest.mark.gpu

F = np.float32
F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
WORD = {F32: (torch.int32, 0x7FC0BEEF), F64: (torch.int64, 0x7FF8DEAD0000BEEF), I32: (torch.int32, -7), I64: (torch.int64, -7),
        U8: (U8, 0x3C)}
TORCH = {np.dtype(np.float32): F32, np.dtype(np.float64): F64, np.dtype(np.int32): I32, np.dtype(np.int64): I64,
         np.dtype(np.uint8): U8}


def _out(g, shape, dtype):
    """A guarded tensor a kernel may write, every word the sentinel of its type."""
    t = g._view(shape, dtype)
    as_int, word = WORD[dtype]
    t.view(as_int).fill_(word)
    return t


def _put(g, a):
    """A guarded tensor holding the host array ``a``."""
    a = np.ascontiguousarray(a)
    t = g._view(a.shape, TORCH[a.dtype])
    t.copy_(torch.from_numpy(a))
    return t


def _host(t):
    return _raw(t.cpu().numpy())


def _kept(t):
    """Which words of a downloaded tensor still hold the pre-fill."""
    return _host(t) == np.array(WORD[t.dtype][1]).astype(_host(t).dtype)


def _bits(a, dtype=F):
    return _raw(np.ascontiguousarray(a, dtype=dtype))


def _masks(ms):
    return np.array([EC.signed(m & K.U64) for m in ms], dtype=np.int64)


# ---- 1. score ------------------------------------------------------------------------------------------------------------------

def _score_key(c):
    gate = c["positions"] is not None
    return (c["NR"], c["NS"], c["MK"], c["min_id"], c["max_distance"] if gate else None)


SCORE_GROUPS = {}
for _c in EC.search_cases() + EC.gate_cases():
    SCORE_GROUPS.setdefault(_score_key(_c), []).append(_c)


@pytest.mark.parametrize("key", sorted(SCORE_GROUPS, key=str), ids=lambda k: "%dx%d-mk%d-id%d-%s" % k)
def test_score_edges(cuda, key):
    """One launch per (shape, MK, gate): a stream per case, then an idle stream that holds the first case's places."""
    NR, NS, MK, min_id, max_distance = key
    cases = list(SCORE_GROUPS[key])
    cases.append(dict(cases[0], active=0, name="idle"))
    S, g = len(cases), Guards(cuda)
    desc = np.full((S, MK, NS, NR), np.nan, dtype=F)
    mask, frame = np.full((S, MK), -7, dtype=np.int64), np.full((S, MK), -7, dtype=np.int32)
    for s, c in enumerate(cases):
        n = c["count"]
        desc[s, :n] = np.transpose(c["En"], (0, 2, 1))
        mask[s, :n], frame[s, :n] = _masks(c["emask"]), c["frame_ids"]
    traj = None
    if max_distance is not None:
        traj = np.tile(np.eye(4), (EC.GATE_FRAMES, S, 1, 1))
        for s, c in enumerate(cases):
            traj[:, s, :3, 3] = c["positions"]
        traj = torch.from_numpy(traj).to(cuda)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    Qn, qmask = dev(np.stack([c["Qn"] for c in cases])), dev(_masks([c["qmask"] for c in cases]))
    count, active = dev(np.array([c["count"] for c in cases], dtype=np.int32)), dev(np.array([c["active"] for c in cases], dtype=np.int32))
    fid = dev(np.array([c["f"] for c in cases], dtype=np.int32))
    desc, mask, frame = dev(desc), dev(mask), dev(frame)
    scores, shifts = _out(g, (S, MK), F32), _out(g, (S, MK), I32)
    _lib.call("loop_score_kernel_wrapper", cuda, S, NR, NS, MK, _p(Qn), _p(qmask), _p(desc), _p(mask), _p(frame), _p(count),
              _p(active), _p(fid), min_id, _p(traj), EC.GATE_FRAMES if traj is not None else 0,
              max_distance if traj is not None else 0.0, _p(scores), _p(shifts))
    got_d, got_s = _host(scores), shifts.cpu().numpy()
    for s, c in enumerate(cases):
        want_d, want_s = K.model_scores(c)
        assert np.array_equal(got_d[s], _bits(want_d)), (c["name"], scores[s].tolist(), want_d)
        assert np.array_equal(got_s[s], want_s), (c["name"], got_s[s], want_s)
    assert np.isposinf(scores[-1].cpu().numpy()).all()                      # the idle stream
    assert g.check() == 2


# ---- 2. select -----------------------------------------------------------------------------------------------------------------

SELECT_GROUPS = {}
for _c in EC.select_cases():
    SELECT_GROUPS.setdefault((_c["MK"], float(_c["threshold"]), _c["stride"]), []).append(_c)


@pytest.mark.parametrize("key", sorted(SELECT_GROUPS), ids=lambda k: "mk%d-thr%g-stride%d" % k)
def test_select_edges(cuda, key):
    MK, threshold, stride = key
    cases, NS = SELECT_GROUPS[key], EC.SELECT_NS
    S, g = len(cases), Guards(cuda)
    table = L.tables(20, NS, 80.0)[2]
    col = lambda k, dt: torch.from_numpy(np.stack([np.asarray(c[k], dtype=dt) for c in cases])).to(cuda)
    scores, shifts, frames = col("scores", F), col("shifts", np.int32), col("frame_ids", np.int32)
    count, active, fid = col("count", np.int32), col("active", np.int32), col("f", np.int32)
    T0_table = torch.from_numpy(table).to(cuda)
    match, score, found = _out(g, (S, 4), I32), _out(g, (S,), F32), _out(g, (S,), I32)
    T0, slot, overflow = _out(g, (S, 4, 4), F64), _out(g, (S,), I32), _put(g, np.zeros(1, dtype=np.int32))
    launch = lambda: _lib.call("loop_select_kernel_wrapper", cuda, S, NS, MK, stride, threshold, _p(scores), _p(shifts),
                               _p(frames), _p(count), _p(active), _p(fid), _p(T0_table), _p(match), _p(score), _p(found),
                               _p(T0), _p(slot), _p(overflow))
    launch()
    want = [M.select(c["scores"], c["shifts"], c["frame_ids"], c["count"], c["active"], c["f"], stride, threshold, MK)
            for c in cases]
    got_T = T0.cpu().numpy()
    for s, (c, w) in enumerate(zip(cases, want)):
        assert tuple(match[s].tolist()) == w["match"], (c["name"], match[s].tolist(), w)
        assert int(_host(score)[s]) == int(_bits([w["score"]])[0]), (c["name"], float(score[s]), w)
        assert int(found[s]) == w["found"] and int(slot[s]) == w["slot"], (c["name"], int(found[s]), int(slot[s]), w)
        pose = np.eye(4) if w["row"] is None else table[w["row"]]
        assert got_T[s].tobytes() == np.ascontiguousarray(pose).tobytes(), c["name"]
    assert int(overflow[0]) == int(any(w["overflow"] for w in want))
    overflow.fill_(1)                                                       # once set, the word is never cleared
    count.fill_(0)
    launch()
    assert int(overflow[0]) == 1
    assert g.check() == 6


# ---- 3. accept -----------------------------------------------------------------------------------------------------------------

ACCEPT = {name: (cfg, rows) for name, cfg, rows in EC.accept_tables()}


def _accept(cuda, cfg, st):
    S, ML, g = len(st["found"]), cfg["ML"], Guards(cuda)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    found, match, score, fid, T = dev(st["found"]), dev(st["match"]), dev(st["score"]), dev(st["f"]), dev(st["T"])
    status, pairs, cost = (dev(st["status"]), dev(st["pairs"]), dev(st["cost"])) if cfg["status"] else (None, None, None)
    log_i, log_T, log_c = _out(g, (S, ML, 4), I32), _out(g, (S, ML, 4, 4), F64), _out(g, (S, ML, 2), F64)
    nlog, over, accepted = _put(g, st["nlog"]), _put(g, np.zeros(1, dtype=np.int32)), _out(g, (S,), I32)
    _lib.call("loop_accept_kernel_wrapper", cuda, S, cfg["n"], ML, _p(found), _p(match), _p(score), _p(fid), _p(T), _p(status),
              _p(pairs), _p(cost), cfg["min_fitness"], cfg["max_mean_cost"], _p(log_i), _p(log_T), _p(log_c), _p(nlog), _p(over),
              _p(accepted))
    want = K.accept_model(cfg, st)
    li, lT, lc = log_i.cpu().numpy(), log_T.cpu().numpy(), log_c.cpu().numpy()
    ki, kT, kc = _kept(log_i), _kept(log_T), _kept(log_c)
    for s, (r, w) in enumerate(zip(st["rows"], want)):
        assert int(accepted[s]) == w["accepted"] and int(nlog[s]) == w["nlog"], (s, r, int(accepted[s]), int(nlog[s]), w)
        rows = np.ones(ML, dtype=bool)
        if w["record"] is not None:
            l = w["nlog"] - 1
            rows[l] = False
            assert li[s, l].tobytes() == w["record"][0].tobytes(), (s, r, li[s, l])
            assert lT[s, l].tobytes() == w["record"][1].tobytes(), (s, r)
            assert lc[s, l].tobytes() == w["record"][2].tobytes(), (s, r, lc[s, l])
        assert ki[s][rows].all() and kT[s][rows].all() and kc[s][rows].all(), (s, r, "another log row was written")
    assert int(over[0]) == int(any(w["overflow"] for w in want))
    assert g.check() == 6
    return want


@pytest.mark.parametrize("S", EC.ACCEPT_S)
def test_accept_edges_at_every_block_size(cuda, S):
    """S = 1, 64, 65, 130: blocks of 64, 64, 128 and 192 threads; one case per stream, cycling through the table."""
    cfg, rows = ACCEPT["main"]
    want = _accept(cuda, cfg, EC.accept_streams(rows, S))
    assert S < len(rows) or {w["accepted"] for w in want} == {0, 1} and any(w["overflow"] for w in want)


@pytest.mark.parametrize("name", [n for n in ACCEPT if n != "main"])
def test_accept_edges_of_every_setting(cuda, name):
    cfg, rows = ACCEPT[name]
    for S in (len(rows), 65):
        _accept(cuda, cfg, EC.accept_streams(rows, S))


# ---- 4. fetch and insert -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", EC.COPY_N)
def test_fetch_edges(cuda, n):
    st, MK, g = EC.fetch_streams(n), EC.COPY_MK, Guards(cuda)
    S = len(st["rows"])
    found, match, db = (torch.from_numpy(st[k]).to(cuda) for k in ("found", "match", "db_cloud"))
    staging = _out(g, (S, n, 3), F32)
    _lib.call("loop_fetch_kernel_wrapper", cuda, S, n, MK, _p(found), _p(match), _p(db), _p(staging))
    got, kept = _host(staging), _kept(staging)
    for s, r in enumerate(st["rows"]):
        want = M.fetch(int(st["found"][s]), st["match"][s], st["db_cloud"][s], MK)
        assert (want is not None) == r["want"]
        if want is None:
            assert kept[s].all(), r["name"]                                 # staging keeps every word
        else:
            assert np.array_equal(got[s], _bits(want)), r["name"]
    assert g.check() == 1


def _insert(cuda, n, NR, NS, with_cloud):
    st, MK, g = EC.insert_streams(n, NR, NS), EC.COPY_MK, Guards(cuda)
    S = len(st["rows"])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    slot, fid, Qn, qmask, cloud = dev(st["slot"]), dev(st["f"]), dev(st["Qn"]), dev(_masks(st["qmask"])), dev(st["cloud"])
    db_desc, db_mask, db_frame = _out(g, (S, MK, NS, NR), F32), _out(g, (S, MK), I64), _out(g, (S, MK), I32)
    db_cloud, count = _out(g, (S, MK, n, 3), F32), _put(g, st["count"])
    _lib.call("loop_insert_kernel_wrapper", cuda, S, n, NR, NS, MK, _p(slot), _p(fid), _p(Qn), _p(qmask),
              _p(cloud) if with_cloud else 0, _p(db_desc), _p(db_mask), _p(db_frame), _p(db_cloud) if with_cloud else 0, _p(count))
    for s, r in enumerate(st["rows"]):
        w = M.insert(int(st["slot"][s]), int(st["f"][s]), st["Qn"][s], st["qmask"][s], st["cloud"][s] if with_cloud else None, MK)
        assert (w is not None) == r["want"]
        others = np.ones(MK, dtype=bool)
        if w is None:
            assert int(count[s]) == r["count"], r["name"]
        else:
            e = w["entry"]
            others[e] = False
            assert np.array_equal(_host(db_desc[s, e]), _bits(w["desc"])), r["name"]      # E[j][r] = Qn[r][j], as words
            assert int(db_mask[s, e]) == EC.signed(w["mask"]) and int(db_frame[s, e]) == w["frame"], r["name"]
            assert int(count[s]) == w["count"] == r["slot"] + 1, r["name"]
            if with_cloud:
                assert np.array_equal(_host(db_cloud[s, e]), _bits(w["cloud"])), r["name"]
        for t in (db_desc, db_mask, db_frame) + ((db_cloud,) if with_cloud else ()):
            assert _kept(t[s])[others].all(), (r["name"], "another entry was written")
    if not with_cloud:
        assert _kept(db_cloud).all()                                        # cloud = None: no cloud is kept
    assert g.check() == 5


@pytest.mark.parametrize("n,shape", list(zip(EC.COPY_N, EC.COPY_SHAPES)))
def test_insert_edges(cuda, n, shape):
    _insert(cuda, n, shape[0], shape[1], True)


def test_insert_without_clouds(cuda):
    _insert(cuda, 683, 3, 63, False)


# ---- 5. build ------------------------------------------------------------------------------------------------------------------

def _build(cuda, streams, n, z_offset, NR=20, NS=60):
    S, g = len(streams), Guards(cuda)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    ring_b, sector_d = (dev(t) for t in L.tables(NR, NS, EC.C.MAX_RANGE)[:2])
    cloud = dev(np.stack([c["cloud"] for c in streams]).astype(F))
    word = lambda k: dev(np.array([c[k] for c in streams], dtype=np.int32))
    lengths, active, restart = word("length"), word("active"), word("restart")
    D, Dn, mask = _out(g, (S, NR, NS), F32), _out(g, (S, NR, NS), F32), _out(g, (S,), I64)
    count, nlog, epoch = (_put(g, np.full(S, v, dtype=np.int32)) for v in (5, 2, 7))
    _lib.call("scan_context_build_kernel_wrapper", cuda, S, n, NR, NS, 0, z_offset, _p(cloud), _p(lengths), _p(ring_b),
              _p(sector_d), _p(D), _p(Dn), _p(mask), _p(active), _p(restart), _p(count), _p(nlog), _p(epoch))
    for s, c in enumerate(streams):
        w = M.build(c["cloud"], c["length"], c["active"], c["restart"], 5, 2, 7, rings=NR, sectors=NS, z_offset=z_offset)
        if w is None:                                                       # an idle stream keeps every word
            assert _kept(D[s]).all() and _kept(Dn[s]).all() and _kept(mask[s:s + 1]).all(), c["name"]
            assert (int(count[s]), int(nlog[s]), int(epoch[s])) == (5, 2, 7), c["name"]
            continue
        assert np.array_equal(_host(D[s]), _bits(w["D"])), c["name"]
        assert np.array_equal(_host(Dn[s]), _bits(w["Dn"])), c["name"]
        assert int(mask[s]) == EC.signed(w["mask"]), c["name"]
        assert (int(count[s]), int(nlog[s]), int(epoch[s])) == (w["count"], w["nlog"], w["epoch"]), c["name"]
    assert g.check() == 6


@pytest.mark.parametrize("n", EC.BUILD_N)
def test_build_edges(cuda, n):
    _build(cuda, EC.build_streams(n), n, 2.0)
    _build(cuda, EC.tiny_streams(n), n, EC.TINY)


# ---- 6. the translation search on planted buffers ------------------------------------------------------------------------------

def _translation(cuda, S, p, up="z", n=64):
    """A detector whose every written buffer of the translation search sits between guard bands, pre-filled."""
    det = L.ScanContextLoopDetector(S, n, sectors=ELC.SECTORS, z_offset=ELC.Z_OFFSET, up=up, max_keyframes=1, device=cuda,
                                    translation=p)
    det._alloc()
    g = Guards(cuda)
    for name in ("ei_img", "ei_occ", "ei_list", "ei_A", "ei_record", "T1"):
        det.bufs[name] = _out(g, tuple(det.bufs[name].shape), det.bufs[name].dtype)
    return det, g


def test_image_refuses_a_shift_outside_the_table(cuda):
    """A shift of -1 and of NS in ``match``: nothing is imaged, the record is zeros and T1 is T0 to the byte; the stream
    between them is imaged as the model says."""
    p, n, NS = dict(ELC.SMALL), 64, ELC.SECTORS
    det, g = _translation(cuda, 3, p)
    b = det.bufs
    rng = np.random.default_rng(5)
    cloud = lambda: np.stack([rng.uniform(-9, 9, n), rng.uniform(-9, 9, n), rng.uniform(-3, 6, n)], axis=1).astype(F)
    stored, query, shifts = [cloud() for _ in range(3)], [cloud() for _ in range(3)], [-1, 7, NS]
    T0 = np.stack([np.eye(4) + 0.01 * rng.normal(size=(4, 4)) for _ in range(3)])
    b["staging"].copy_(torch.from_numpy(np.stack(stored)))
    b["cloud"].copy_(torch.from_numpy(np.stack(query)))
    b["lengths"].fill_(n)
    b["found"].fill_(1)
    b["match"].copy_(torch.tensor([[1, 0, 0, s] for s in shifts], dtype=torch.int32))
    b["T0"].copy_(torch.from_numpy(T0))
    det.image()
    out = EM.search(stored[1], query[1], 7, NS, p, T0=T0[1])
    img, occ = b["ei_img"].cpu().numpy(), b["ei_occ"].cpu().numpy()
    for s in (0, 2):
        assert not img[s].any() and not occ[s].any() and _kept(b["ei_list"][s]).all()
    assert np.array_equal(img[1, 0], out["E"]) and np.array_equal(img[1, 1:], out["Q"])
    assert occ[1, 0] == out["occ_e"] and np.array_equal(occ[1, 1:], out["occ_q"])
    for k in range(len(out["Q"])):
        i, j = np.nonzero(out["Q"][k])
        want = set((i | (j << 8) | (out["Q"][k][i, j].astype(np.int64) << 16)).tolist())
        assert set(b["ei_list"][1, k, :occ[1, 1 + k]].tolist()) == want
        assert _kept(b["ei_list"][1, k, occ[1, 1 + k]:]).all()
    det.agreement()
    A = b["ei_A"].cpu().numpy()
    assert not A[0].any() and not A[2].any() and np.array_equal(A[1], out["A"])
    det.choose()
    rec, T1 = b["ei_record"].cpu().numpy(), b["T1"].cpu().numpy()
    for s in (0, 2):
        assert rec[s].tolist() == [0] * 8 and T1[s].tobytes() == T0[s].tobytes()
    assert rec[1].tolist() == [out["record"][k] for k in EM.RECORD] + [0]
    assert T1[1].tobytes() == np.ascontiguousarray(out["T1"]).tobytes()
    assert g.check() == 6


@pytest.mark.parametrize("window,tolerance", [(8, 1), (8, 255), (16, 1), (16, 255)])
def test_agreement_on_planted_lists(cuda, window, tolerance):
    """C = 289 and 1089 candidates (no multiple of 64 or 256); occ of -1 and G G + 1; list words with i = G and with j = G;
    level 255 against level 1; a stream without a match keeps the pre-fill."""
    G, Y = 8, 3
    p = dict(ELC.SMALL, cells=G, window=window, tolerance=tolerance, yaw_half=1)
    S = 4
    det, g = _translation(cuda, S, p)
    b = det.bufs
    rng = np.random.default_rng(window + tolerance)
    E = rng.choice(np.array([0, 1, 2, 128, 255], dtype=np.uint8), size=(S, G, G))
    Q = rng.choice(np.array([0, 0, 1, 3, 255], dtype=np.uint8), size=(S, Y, G, G))
    Q[:, :, 0, 0], E[:, 0, 0] = 255, 1                                      # q = 255 against level 1
    img = np.concatenate([E[:, None], Q], axis=1)
    lists = np.full((S, Y, G * G), -7, dtype=np.int32)
    occ = np.zeros((S, 1 + Y), dtype=np.int32)
    for s in range(S):
        occ[s, 0] = (E[s] > 0).sum()
        for k in range(Y):
            i, j = np.nonzero(Q[s, k])
            words = (i | (j << 8) | (Q[s, k][i, j].astype(np.int64) << 16)).astype(np.int32)
            bad = np.array([G | (0 << 8) | (9 << 16), 0 | (G << 8) | (9 << 16), 255 | (255 << 8) | (255 << 16)], dtype=np.int32)
            both = np.concatenate([words[:5], bad, words[5:]])              # the words to skip sit inside the list
            assert 8 < len(both) <= G * G
            pad = np.full(G * G - len(both), bad[0], dtype=np.int32)
            lists[s, k] = np.concatenate([both, pad])
            occ[s, 1 + k] = len(both)
    occ[1, 1:] = -1                                                         # clamped to 0: every score 0
    occ[2, 1:] = G * G + 1                                                  # clamped to G G: the padding is skipped word by word
    found = [1, 1, 1, 0]
    b["ei_img"].copy_(torch.from_numpy(img))
    b["ei_occ"].copy_(torch.from_numpy(occ))
    b["ei_list"].copy_(torch.from_numpy(lists))
    b["found"].copy_(torch.tensor(found, dtype=torch.int32))
    det.agreement()
    A = b["ei_A"].cpu().numpy()
    for s in (0, 2):
        want = EM.scores(Q[s], E[s], window, tolerance)
        assert want.shape == (Y, 2 * window + 1, 2 * window + 1) and want.any()
        assert np.array_equal(A[s], want), s
    assert EM.scores(Q[0], E[0], window, tolerance)[0, window, window] >= (1 if tolerance == 255 else 0)
    assert not A[1].any() and _kept(b["ei_A"][3]).all()
    assert np.array_equal(b["ei_img"].cpu().numpy(), img) and np.array_equal(b["ei_occ"].cpu().numpy(), occ)
    assert g.check() == 6


CHOOSE = [(8, 0.5, "z"), (16, 0.5, "-y"), (8, 0.0, "z"), (16, 0.0, "-y")]


@pytest.mark.parametrize("window,min_agreement,up", CHOOSE)
def test_choose_on_planted_scores(cuda, window, min_agreement, up):
    """Y C = 867 and 3267 entries: equal maxima 256 apart, across k and at the last index; all zero; the acceptance at its
    bound (L = 4, min(occ) = 10: 20 against 19) and at min_agreement = 0 with A = 0; b = 0 for both ``up``."""
    Y, L_, NS = 3, 4, ELC.SECTORS
    side = 2 * window + 1
    C_, total = side * side, 3 * side * side
    p = dict(ELC.SMALL, cells=8, window=window, tolerance=L_, yaw_half=1, min_agreement=min_agreement)
    b0 = window                                                             # the column of b = 0
    at = lambda k, a, b_: (k * side + a + window) * side + b_ + window
    plants = [("tie_256", {at(0, -window, 0): 50, at(0, -window, 0) + 256: 50}), ("tie_across_k", {at(0, 2, 0): 50, at(2, 2, 0): 50}),
              ("last", {total - 1: 50}), ("zero", {}), ("at_bound", {at(1, 3, 0): 20}), ("below_bound", {at(1, 3, 0): 19}),
              ("one", {at(2, -1, 0): 1}), ("tie_last", {at(1, 0, 0): 50, total - 1: 50})]
    S = len(plants) + 1
    det, g = _translation(cuda, S, p, up)
    b = det.bufs
    A = np.zeros((S, Y, side, side), dtype=np.int32)
    for s, (_, plant) in enumerate(plants):
        for i, v in plant.items():
            A[s].reshape(-1)[i] = v
    A[-1] = 99                                                              # the stream without a match
    occ = np.full((S, 1 + Y), 10, dtype=np.int32)
    occ[:, 2] = 12
    shifts = [(7 * s + 3) % NS for s in range(S)]
    T0 = np.stack([M.start_pose(sh, NS, up) for sh in shifts])
    b["ei_A"].copy_(torch.from_numpy(A))
    b["ei_occ"].copy_(torch.from_numpy(occ))
    b["found"].copy_(torch.tensor([1] * (S - 1) + [0], dtype=torch.int32))
    b["match"].copy_(torch.tensor([[1, 0, 0, sh] for sh in shifts], dtype=torch.int32))
    b["T0"].copy_(torch.from_numpy(T0))
    det.choose()
    rec, T1 = b["ei_record"].cpu().numpy(), b["T1"].cpu().numpy()
    decided = {}
    for s, (name, _) in enumerate(plants):
        w = EM.choose(A[s], occ[s, 1:], occ[s, 0], window, L_, min_agreement)
        decided[name] = w
        assert rec[s].tolist() == [w[k] for k in EM.RECORD] + [0], (name, rec[s].tolist(), w)
        assert T1[s].tobytes() == np.ascontiguousarray(EM.seed(w, shifts[s], T0[s], NS, p, up)).tobytes(), name
    assert rec[-1].tolist() == [0] * 8 and T1[-1].tobytes() == T0[-1].tobytes()
    assert (decided["tie_256"]["a"], decided["tie_across_k"]["k"], decided["tie_last"]["k"]) == (-window, 0, 1)
    assert (decided["last"]["k"], decided["last"]["a"], decided["last"]["b"]) == (2, window, window)
    assert decided["zero"]["found"] == 0 and decided["one"]["found"] == int(min_agreement == 0.0)
    assert (decided["at_bound"]["found"], decided["below_bound"]["found"]) == ((1, 0) if min_agreement else (1, 1))
    assert decided["at_bound"]["b"] == 0 and np.array_equal(b["ei_A"].cpu().numpy(), A)
    assert g.check() == 6


# ---- 7. raw mode with loop= ----------------------------------------------------------------------------------------------------

def test_raw_mode_with_loop_keeps_every_output(cuda):
    """Raw KITTI sweeps of two streams of different lengths with ``loop=``: the detector is made with ``up="-y"``, receives
    the survivor counts as lengths, stores the descriptor of the tapped cloud, is emptied by a stream's restart, and changes no
    odometry output."""
    import test_gpu_raw_stream as R
    from pwclonet_pylidarslam_amd.odometry import StreamingOdometry
    S, T = 2, 4
    seqs = [R._sweeps(51 + s, T) for s in range(S)]
    net = R._net(cuda)
    make = lambda **kw: StreamingOdometry(net, streams=S, max_frames=8, graph=True, per_stream=True,
                                          sweeps=dict(dataset="kitti", capacity=R.CAP, tr=R._trs(S)),
                                          backend=dict(source="network", max_loops=4, iters=6), **kw)
    plain, looped = make(), make(loop=dict(min_id_distance=2, max_keyframes=8, verify=None))
    schedule = [((1, 1), (0, 0)), ((1, 1), (0, 0)), ((1, 1), (0, 1)), ((1, 1), (0, 0))]     # stream 1 restarts at call 2
    stored = [[], []]
    with torch.no_grad():
        for k, (active, restart) in enumerate(schedule):
            rows = [seqs[0][k], seqs[1][k][:6000 + 500 * k]]                # stream 1 keeps fewer than num_points rows
            batch, lengths = R._batch(rows, cuda)
            a = plain.step_sweeps(batch, lengths, active=list(active), restart=list(restart))
            b = looped.step_sweeps(batch, lengths, active=list(active), restart=list(restart))
            assert (a is None and b is None) or torch.equal(a, b), k
            assert torch.equal(plain.frame_counts(), looped.frame_counts()), k
            det = looped.loop_detector()
            assert det.up == "-y"
            survivors = looped.survivor_counts()
            assert torch.equal(det.bufs["lengths"], survivors) and torch.equal(survivors, plain.survivor_counts())
            tapped = looped._tapped[:, :looped.num_points, :3].contiguous().cpu().numpy()
            for s in range(S):
                if restart[s]:
                    stored[s] = []
                stored[s].append(M.descriptor(tapped[s], length=int(survivors[s]), up="-y"))
            assert det.counts().tolist() == [len(stored[0]), len(stored[1])], k
    assert 0 < int(survivors[1]) < looped.num_points and int(survivors[0]) != int(survivors[1])
    assert det.counts().tolist() == [4, 2]
    for s in range(S):
        db = det.database(s)
        assert db["frame_id"].tolist() == list(range(len(stored[s])))
        for e, (_, dn, m) in enumerate(stored[s]):
            assert np.array_equal(_host(db["Dn"][e].contiguous()), _bits(dn)), (s, e)
            assert int(db["mask"][e]) == EC.signed(m), (s, e)
            assert m != 0
    for name in ("relative_poses", "trajectory", "optimized_trajectory"):
        for s in range(S):
            assert torch.equal(getattr(plain, name)(stream=s), getattr(looped, name)(stream=s)), (name, s)
    assert plain.loop_detector() is None and not det.overflowed()
    torch.cuda.synchronize()
    assert _lib.load().pwclo_last_error() == 0
