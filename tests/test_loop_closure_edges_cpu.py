"""The edge cases of the loop detector's kernels without a GPU: every named case of
tests/loop_closure_edge_cases.py takes the branch it is named after, asserted on the model; the search cases with a real
winner carry the fp64 margins tests/test_loop_closure_cpu.py asks of ``search_case``; and a second implementation written the
way the kernels work (tests/loop_closure_second.py) equals the model on every case and differs on at least one for each of
eighteen planted faults.  ``fault_table()`` is what profiles/loop_closure_edges/README.md records."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_closure_cases as C          # noqa: E402
import loop_closure_edge_cases as EC    # noqa: E402
import loop_closure_model as M          # noqa: E402
import loop_closure_second as K         # noqa: E402

F = np.float32
SEARCH = EC.search_cases()
GATE = EC.gate_cases()
SELECT = EC.select_cases()
ACCEPT = EC.accept_tables()


def _i32(v):
    return int(np.array([v], dtype=F).view(np.int32)[0])


# ---- every case takes its branch -----------------------------------------------------------------------------------------------

def test_search_shapes_counts_and_rules_are_all_there():
    assert {(c["NR"], c["NS"]) for c in SEARCH} == set(EC.SHAPES) and len(EC.SHAPES) == 6
    for shape in EC.SHAPES:
        mine = [c for c in SEARCH if (c["NR"], c["NS"]) == shape]
        assert {(c["count"], c["MK"]) for c in mine} >= {(3, 3), (3, 4), (4, 4), (4, 5), (5, 5), (5, 6)}, shape
        assert {c["rule"] for c in mine} >= {"full", "bit0_one_overlap", "bit_last_to_bit0", "bit_last_same", "query_mask0",
                                             "entry_mask0", "disjoint", "last_shift", "equal", "equal_twice"}
        assert (shape[1] % 2 == 1) != any(c["rule"] == "period" for c in mine)
    assert {c["MK"] for c in SEARCH} == {1, 2, 3, 4, 5, 6} and {c["count"] for c in SEARCH} == {1, 3, 4, 5}
    assert any(c["NS"] == 64 and c["qmask"] >> 63 for c in SEARCH)               # bit 63 of a mask runs in a search


@pytest.mark.parametrize("c", SEARCH, ids=lambda c: c["name"])
def test_search_case_takes_its_branch(c):
    scores, shifts = K.model_scores(c)
    w, NS = c["want"], c["NS"]
    ans = K.answer_model(c)[2]
    if w.get("all_inf"):
        assert np.isposinf(scores).all() and not shifts.any() and ans[0] == M.NO_MATCH and ans[1] == 0x7F800000
        return
    if w.get("inf_at"):
        assert np.isposinf(scores[w["at"]]) and shifts[w["at"]] == 0                # disjoint at every shift: inf, shift 0
    e = w["entry"]
    d = M.distances(c["Qn"], c["qmask"], c["En"][e:e + 1], [c["emask"][e] & K.U64])[0]
    if "overlaps" in w:
        assert np.isfinite(d).sum() == w["overlaps"] and shifts[e] == w["shift"]     # the masks alone decide the shift
    elif c["NR"] == 1:
        assert (d == 0).all() and shifts[e] == 0 and scores[e] == 0                 # one ring: every shift ties, the lowest wins
    else:
        assert shifts[e] == w["shift"] and scores[e] < 5e-3
        if "tied_shift" in w:
            assert _i32(d[w["tied_shift"]]) == _i32(d[w["shift"]]) and w["tied_shift"] > w["shift"]      # equal to the bit
    if c["NR"] > 1:
        assert ans[0][:2] == (1, e) and ans[0][3] == shifts[e]
        if "tied_entry" in w:
            t = e + w["tied_entry"]
            assert _i32(scores[t]) == _i32(scores[e]) and shifts[t] == shifts[e]
    else:
        assert ans[0][0] == 1 and ans[0][1] <= e and scores[ans[0][1]] == 0         # the lowest of the tied entries


@pytest.mark.parametrize("c", GATE, ids=lambda c: c["name"])
def test_gate_case_takes_its_branch(c):
    scores, _ = K.model_scores(c)
    assert np.isfinite(scores[:c["count"]]).astype(int).tolist() == c["want"]["eligible"], scores
    assert np.isposinf(scores[c["count"]:]).all()


def test_select_sizes_and_rules_are_all_there():
    assert {c["MK"] for c in SELECT} == set(EC.SELECT_MK)
    for rule, least in (("tie_stride", 257), ("tie_2_257", 258), ("tie_10_300", 513), ("nan_first", 255), ("min_last", 1)):
        assert {c["MK"] for c in SELECT if c["rule"] == rule} == {m for m in EC.SELECT_MK if m >= least}, rule
    for c in SELECT:
        assert ((c["shifts"] >= 0) & (c["shifts"] < c["NS"])).all() and np.isposinf(c["scores"][max(c["count"], 0):]).all()


@pytest.mark.parametrize("c", SELECT, ids=lambda c: c["name"])
def test_select_case_takes_its_branch(c):
    o = M.select(c["scores"], c["shifts"], c["frame_ids"], c["count"], c["active"], c["f"], c["stride"], c["threshold"], c["MK"])
    w = c["want"]
    if "entry" in w:
        assert o["match"][1] == w["entry"], o
        if w["entry"] >= 0:
            assert o["match"][2:] == (int(c["frame_ids"][w["entry"]]), int(c["shifts"][w["entry"]]))
        else:
            assert o["match"] == M.NO_MATCH and o["row"] is None
    for key in ("found", "slot", "overflow"):
        if key in w:
            assert o[key] == w[key], (key, o)
    assert (o["row"] is not None) == bool(o["found"]) and o["match"][0] == o["found"]
    if "score_bits" in w:
        assert _i32(o["score"]) == w["score_bits"]
    if c["rule"].startswith("tie_"):
        at = np.nonzero(c["scores"] == c["scores"].min())[0]
        assert len(at) == 2 and at[0] == w["entry"]


def test_accept_tables_take_their_branches():
    names = set()
    for name, cfg, rows in ACCEPT:
        st = EC.accept_streams(rows, len(rows))
        for s, (r, o) in enumerate(zip(rows, K.accept_model(cfg, st))):
            names.add(r["name"])
            if r["want"] == "overflow":
                assert (o["accepted"], o["overflow"], o["nlog"], o["record"]) == (0, True, r["nlog"], None), (name, r)
                continue
            assert o["accepted"] == r["want"] and not o["overflow"], (name, r, o)
            assert o["nlog"] == r["nlog"] + r["want"] and (o["record"] is not None) == bool(r["want"])
            if r["want"]:
                li, lT, lc = o["record"]
                pairs, cost = (r["pairs"], r["cost"]) if cfg["status"] else (0, 0.0)
                assert li.tolist() == [100 + s, 500 + s, s % 60, pairs] and lT.tobytes() == st["T"][s].tobytes()
                assert lc.tobytes() == np.array([np.float64(st["score"][s]), cost]).tobytes()
    assert len(names) >= 30
    mf, n, whole = EC.product_off_an_integer()
    assert mf * n != whole and abs(mf * n - whole) < 1e-9                          # the decimal product is the integer


def test_fetch_and_insert_rows_take_their_branches():
    MK = EC.COPY_MK
    for n in EC.COPY_N:
        st = EC.fetch_streams(n)
        for s, r in enumerate(st["rows"]):
            got = M.fetch(int(st["found"][s]), st["match"][s], st["db_cloud"][s], MK)
            assert (got is not None) == r["want"], r
            if r["want"]:
                assert got.tobytes() == st["db_cloud"][s, r["entry"]].tobytes()
        assert np.isnan(st["db_cloud"]).any() and (st["db_cloud"].view(np.int32) == EC.INT_MIN).any() or n == 1
    for n, (NR, NS) in zip(EC.COPY_N, EC.COPY_SHAPES):
        st = EC.insert_streams(n, NR, NS)
        for s, r in enumerate(st["rows"]):
            got = M.insert(int(st["slot"][s]), int(st["f"][s]), st["Qn"][s], st["qmask"][s], st["cloud"][s], MK)
            assert (got is not None) == r["want"], r
            if r["want"]:
                assert got["count"] == r["slot"] + 1 and got["desc"].shape == (NS, NR) and got["mask"] == r["mask"]
                assert all(_i32(got["desc"][j, q]) == _i32(st["Qn"][s, q, j]) for j in (0, NS - 1) for q in (0, NR - 1))
        assert any(r["mask"] >> 63 for r in st["rows"])
    assert [3 * n for n in EC.COPY_N] == [3, 2046, 2049, 4098] and EC.COPY_SHAPES[-1][0] * EC.COPY_SHAPES[-1][1] == 4096


@pytest.mark.parametrize("n", EC.BUILD_N)
def test_build_cases_take_their_branches(n):
    streams = {c["name"]: c for c in EC.build_streams(n)}
    out = {k: M.build(c["cloud"], c["length"], c["active"], c["restart"], 5, 2, 7, rings=20, sectors=60)
           for k, c in streams.items()}
    for a in (0, 1, 2):
        for r in (0, 1, 2):
            o = out["words_a%d_r%d" % (a, r)]
            assert (o is None) == (a == 0)
            if o is not None:
                assert (o["count"], o["nlog"], o["epoch"]) == ((0, 0, 8) if r else (5, 2, 7))
    for length in (EC.INT_MIN, -1, 0):
        assert out["length_%d" % length]["mask"] == 0 and not out["length_%d" % length]["D"].any()
    assert out["length_%d" % n]["mask"] != 0
    assert out["length_%d" % (n + 1)]["D"].tobytes() == out["length_%d" % n]["D"].tobytes()
    assert out["all_dropped"]["mask"] == 0 and not out["all_dropped"]["D"].any()
    one = out["one_cell"]
    assert (one["D"] > 0).sum() == 1 and bin(one["mask"]).count("1") == 1
    assert one["D"].max() == (streams["one_cell"]["cloud"][:, 2] + F(2.0)).max()
    huge = out["height_overflows"]                                                  # the model decides: norm inf, Dn 0, bit set
    assert huge["D"].max() == F(2.0e19) and np.isfinite(huge["D"]).all() and not huge["Dn"].any() and huge["mask"] == one["mask"]
    beside = out["height_zero_and_beside"]
    assert beside["D"].max() == F(2.0 ** -23) and (beside["D"] > 0).sum() == 1
    tiny = {c["name"]: M.descriptor(c["cloud"], 20, 60, z_offset=EC.TINY) for c in EC.tiny_streams(n)}
    assert not tiny["sum_zero"][0].any() and not tiny["sum_below_zero"][0].any()
    sub = tiny["sum_subnormal"]                                                     # D holds the subnormal; its square is 0
    assert sub[0].max() == np.nextafter(F(0), F(1)) and sub[2] == 0 and not sub[1].any()
    assert tiny["subnormal_z"][0].max() == F(EC.TINY) + F(2.0 ** -140) and tiny["subnormal_z"][2] == 0


# ---- margins of the search cases with a real winner -----------------------------------------------------------------------------

@pytest.mark.parametrize("c", [c for c in SEARCH if not c["tie"] and "entry" in c["want"] and c["want"]["entry"] >= 0],
                         ids=lambda c: c["name"])
def test_search_case_has_fp64_margins(c):
    """The rule of tests/test_loop_closure_cpu.py: the winner and its shift lead their runners-up in fp64 by more than 4 x the
    fp32 model's own error, which itself stays within NR NS 2^-23.  A planted tie has margin 0 and is not here."""
    masks = [m & K.U64 for m in c["emask"]]
    d32, d64 = M.distances(c["Qn"], c["qmask"], c["En"], masks), M.distances64(c["Qn"], c["qmask"], c["En"], masks)
    assert np.array_equal(np.isfinite(d32), np.isfinite(d64))
    fin = np.isfinite(d64)
    assert np.abs(d32[fin] - d64[fin]).max() <= c["NR"] * c["NS"] * 2.0 ** -23
    entry, shift, err = C.margins(c["Qn"], c["qmask"], c["En"], masks)
    assert shift > 4 * err and (c["count"] == 1 or entry > 4 * err), (entry, shift, err)
    best = d64.min(axis=1)
    assert int(best.argmin()) == c["want"]["entry"] and int(d64[c["want"]["entry"]].argmin()) == c["want"]["shift"]


# ---- the second implementation and its faults ----------------------------------------------------------------------------------

def _copy_answers(fault, model):
    """Every fetch, insert and build-word case -> {name: answer}."""
    out, MK = {}, EC.COPY_MK
    for n in EC.COPY_N:
        st = EC.fetch_streams(n)
        for s, r in enumerate(st["rows"]):
            args = (int(st["found"][s]), st["match"][s], st["db_cloud"][s], MK)
            got = M.fetch(*args) if model else K.fetch(*args, fault=fault)
            out["fetch-%s-n%d" % (r["name"], n)] = None if got is None else got.tobytes()
    for n, (NR, NS) in zip(EC.COPY_N, EC.COPY_SHAPES):
        st = EC.insert_streams(n, NR, NS)
        for s, r in enumerate(st["rows"]):
            args = (int(st["slot"][s]), int(st["f"][s]), st["Qn"][s], st["qmask"][s], st["cloud"][s], MK)
            if model:
                got = M.insert(*args)
                count = int(st["count"][s]) if got is None else got["count"]
            else:
                got, count = K.insert(*args, int(st["count"][s]), fault=fault)
            key = None if got is None else (got["entry"], got["desc"].tobytes(), got["mask"], got["frame"], got["cloud"].tobytes())
            out["insert-%s-n%d" % (r["name"], n)] = (key, count)
    for a in (0, 1, 2):
        for r in (0, 1, 2):
            out["build-words_a%d_r%d" % (a, r)] = M.build_words(a, r, 5, 2, 7) if model else K.build_words(a, r, 5, 2, 7, fault)
    return out


def _accept_differs(tables, fault):
    out = []
    for name, cfg, rows in tables:
        st = EC.accept_streams(rows, len(rows))
        want, got = K.accept_model(cfg, st), K.accept(cfg, st, fault)
        out += ["accept-%s-%s" % (name, r["name"]) for s, r in enumerate(rows) if not K.same_accept(want[s:s + 1], got[s:s + 1])]
    return out


def caught_by(fault, cases, tables, copies=True):
    """The names of the cases on which the second implementation with ``fault`` differs from the model."""
    out = [c["name"] for c in cases if K.answer_second(c, fault) != K.answer_model(c)]
    out += _accept_differs(tables, fault)
    if copies:
        want, got = _copy_answers(None, True), _copy_answers(fault, False)
        out += [k for k in want if want[k] != got[k]]
    return out


def fault_table():
    """-> [(fault, what, cases of this file that catch it, restated inputs of the earlier files that catch it)].  The earlier
    files ran fetch, insert and build's words through ``process()`` alone; those calls are not restated, so for the faults of
    the copies and of build the last column counts nothing (the README says which of them the earlier files would notice)."""
    new, old = SEARCH + GATE + SELECT, EC.prior_cases()
    return [(f, what, caught_by(f, new, ACCEPT), caught_by(f, old, EC.prior_accept(), copies=False))
            for f, what in sorted(K.FAULTS.items())]


def test_second_implementation_equals_the_model():
    assert caught_by(None, SEARCH + GATE + SELECT, ACCEPT) == []
    for S in EC.ACCEPT_S:                                                           # the launches of the GPU file
        st = EC.accept_streams(ACCEPT[0][2], S)
        assert K.same_accept(K.accept_model(ACCEPT[0][1], st), K.accept(ACCEPT[0][1], st))


@pytest.mark.parametrize("fault", sorted(K.FAULTS))
def test_every_planted_fault_is_caught(fault):
    assert caught_by(fault, SEARCH + GATE + SELECT, ACCEPT), K.FAULTS[fault]


if __name__ == "__main__":
    for f, what, new, old in fault_table():
        print("| %d | %s | %d | %s | %d |" % (f, what, len(new), ", ".join(sorted(new)[:3]), len(old)))
