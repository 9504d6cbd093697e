"""The conditions of tests/voxel_map_cases.py, checked on the model alone (tests/voxel_map_model.py): every case reaches the
edge it names and tells the model from the planted fault that edge is about, so that tests/test_gpu_voxel_map_edges.py
cannot pass by missing it.  Nothing is left out of a comparison: there is no band and no skip list."""
import functools

import numpy as np
import pytest

import icp_model as model
import voxel_map_cases as C
import voxel_map_model as vm

EXT_VOX = pytest.mark.parametrize("extent, voxel", list(zip(C.ANISO, C.VOXELS)) + [(C.ANISO[0], 2.0)],
                                  ids=lambda v: C.ext_id(v) if isinstance(v, tuple) else str(v))


def _world(f, s=0):
    return vm.to32(vm.pose_apply(f["W"][s], f["cloud"][s]))


def _check_model(sc):
    """What holds for every scenario: the map does not depend on the processing order, and the lookup is the brute-force
    nearest wherever that is within one voxel (of the queries that are storable: the others have no candidate by rule)."""
    grids = C.model_end(sc)[0]
    for order_seed in (None, 3):
        S = sc["frames"][0]["cloud"].shape[0]
        other = [vm.Grid(sc["extent"], sc["voxel"]) for _ in range(S)]
        for k, f in enumerate(sc["frames"]):
            n = f["cloud"].shape[1]
            order = np.arange(n)[::-1] if order_seed is None else np.random.default_rng([order_seed, k]).permutation(n)
            for s, g in enumerate(other):
                g.insert(f["cloud"][s], f["normals"][s], f["W"][s], order)
                g.seq += 1
        for g, o in zip(grids, other):
            assert np.array_equal(g.coord, o.coord) and np.array_equal(g.keys, o.keys)
            assert np.array_equal(g.points.view(np.int32), o.points.view(np.int32))
            assert np.array_equal(g.normals.view(np.int32), o.normals.view(np.int32))
    if sc["queries"] is not None:
        for s, g in enumerate(grids):
            dist = g.lookup(sc["queries"][s])[2]
            brute = vm.brute_nearest(g, sc["queries"][s])
            ok = vm.half_index(sc["queries"][s], sc["voxel"])[1]
            near = ok & (brute <= np.float32(sc["voxel"]))
            assert np.array_equal(dist[near], brute[near]) and (dist[~near] > np.float32(sc["voxel"])).all()
            assert np.isinf(dist[~ok]).all()


# ---- anisotropic extents -----------------------------------------------------------------------------------------------------

@EXT_VOX
def test_anisotropic_walk_rejects_on_every_axis_and_tells_the_index_faults(extent, voxel):
    sc = C.aniso_walk(extent, voxel)
    _check_model(sc)
    rc = C.reach(extent, voxel)
    for f in sc["frames"]:
        for s in range(f["cloud"].shape[0]):
            w = _world(f, s)
            with np.errstate(invalid="ignore"):
                out = np.abs(w.astype(np.float64) - f["W"][s][:3, 3]) >= rc
            for a in range(3):                                          # rows that this axis alone rejects
                assert (out[:, a] & ~out[:, (a + 1) % 3] & ~out[:, (a + 2) % 3]).sum() >= 5, a
    grids, _, looks = C.model_end(sc)
    assert all(len(g.map_points()["keys"]) > 100 for g in grids)
    hit = looks[0][0] >= 0
    assert hit.sum() > 100 and (~hit).sum() > 40
    assert C.differs(sc, "insert_cell_xy") and C.differs(sc, "lookup_cell_xy")
    square = dict(sc, extent=(extent[0], extent[0], extent[2]))         # what the suite had: nx == ny hides both
    assert not C.differs(square, "insert_cell_xy") and not C.differs(square, "lookup_cell_xy")


# ---- wraps -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("direction", list(C.DIRECTIONS))
@EXT_VOX
def test_wrap_walks_reclaim_stale_cells_on_every_axis_and_sign(extent, voxel, direction):
    sc = C.wrap_walk(extent, voxel, direction)
    _check_model(sc)
    d = np.array(sc["direction"])
    for k, grids, slot, before in C.model_frames(sc):
        g = grids[0]
        assert (slot >= 0).all()
        if k == 0:
            continue
        taken = np.flatnonzero((before[0] != vm.EMPTY) & (before[0] != g.coord))
        assert len(taken) >= 1, (direction, k)
        moved = vm.unpack(g.coord[taken]) - vm.unpack(before[0][taken])
        assert (moved % np.array(extent) == 0).all()                    # the new owner aliases onto the old one's cell
        for a in np.flatnonzero(d):
            assert (np.sign(moved[:, a]) == d[a]).any(), (direction, k, a)
        keys = g.keys[taken]
        assert ((keys == vm.EMPTY) | (keys >> 32 == k)).all()           # the eight keys were emptied: only this frame's stand
        assert (keys != vm.EMPTY).any()
    assert C.differs(sc, "insert_cell_xy")


# ---- the ends of the range ---------------------------------------------------------------------------------------------------

RANGE = [(e, v, end, axes) for (e, v) in zip(C.ANISO, C.VOXELS) for end in ("low", "high") for axes in ((0, 1, 2), (0,), (1,), (2,))]


@functools.lru_cache(maxsize=None)
def _range(extent, voxel, end, axes):
    return C.range_end(extent, voxel, end, axes)


@pytest.mark.parametrize("extent, voxel, end, axes", RANGE)
def test_range_end_rows_are_stored_and_refused_by_the_range_alone(extent, voxel, end, axes):
    sc = _range(extent, voxel, end, axes)
    _check_model(sc)
    f = sc["frames"][0]
    g = vm.Grid(extent, voxel)
    w, slot, _ = g.slots(f["cloud"][0], f["W"][0])
    h, ok = vm.half_index(w, voxel)
    assert np.array_equal(slot >= 0, sc["stored"]) and sc["stored"].any() and (~sc["stored"]).any()
    assert np.array_equal(h[ok], sc["h"][ok]) and np.array_equal(ok, sc["stored"])
    assert (np.abs(w.astype(np.float64) - f["W"][0][:3, 3]) < C.reach(extent, voxel)).all()     # the box rule refuses none
    named = (C.H_LO, C.H_LO + 1) if end == "low" else (C.H_HI - 1, C.H_HI)
    for a in axes:
        assert set(np.unique(sc["h"][sc["stored"], a])) == set(named)
        beyond = C.H_LO - 1 if end == "low" else C.H_HI + 1
        assert (sc["h"][~sc["stored"]] == beyond).any(axis=1).all()
    cell, octant, dist = C.model_end(sc)[2][0]
    n = len(sc["stored"])
    kept = C.model_end(sc)[0][0].points[np.maximum(slot, 0) >> 3, np.maximum(slot, 0) & 7]
    won = sc["stored"] & (kept == w).all(axis=1)                        # rows share their octants; the lowest one stays
    assert won.sum() == len(np.unique(slot[sc["stored"]])) and (dist[:n][won] == 0).all()  # found in voxels -2^20 and 2^20 - 1
    assert (cell[:n][sc["stored"]] >= 0).all() and (dist[:n][sc["stored"]] <= np.float32(voxel / 4 * np.sqrt(3))).all()
    c = vm.half_index(sc["queries"][0][:n], voxel)[0] >> 1
    for a in axes:
        assert (c[sc["stored"], a] == (-vm.BIAS if end == "low" else vm.BIAS - 1)).all()
    assert (cell[2 * n:] == -1).all()                                   # the opposite end: nothing within 27 voxels


def test_a_coordinate_out_of_range_aliases_onto_a_stored_voxel_where_the_period_divides_the_range():
    """Without vm_voxel_in_range the packed word of a neighbour at -2^20 - 1 or 2^20 spills into the next field and equals
    the word of a voxel at the opposite end; the cell is the same where N_a divides 2^21.  Every anisotropic extent has
    such an axis among x and y; on z the spill sets bit 63, which no stored word has."""
    caught = set()
    for extent, voxel, end, axes in RANGE:
        if len(axes) == 1:
            if C.differs(_range(extent, voxel, end, axes), "no_range"):
                caught.add((extent, end, axes[0]))
    want = {(e, end, a) for e in C.ANISO for end in ("low", "high") for a in (0, 1) if e[a] & (e[a] - 1) == 0}
    assert caught == want and {e for e, _, _ in caught} == set(C.ANISO)


@EXT_VOX
def test_rows_around_zero_go_through_floor_shift_and_mask_of_negative_half_indices(extent, voxel):
    sc = C.zero_straddle(extent, voxel)
    _check_model(sc)
    w = sc["frames"][0]["cloud"][0]
    h, ok = vm.half_index(w, voxel)
    assert ok.all()
    want_h = np.array([0, -1, 0, -1, -1, -2, 0, 0, 1])                  # TINY, -TINY, 1e-30, -1e-30, -half, -voxel, -0., 0., half
    assert np.array_equal(h, want_h[sc["idx"]])
    assert np.array_equal(h >> 1, np.array([0, -1, 0, -1, -1, -1, 0, 0, 0])[sc["idx"]])
    assert np.array_equal(h & 1, np.array([0, 1, 0, 1, 1, 0, 0, 0, 1])[sc["idx"]])
    slot = C.model_end(sc)[1][0][0]
    for a in range(3):
        at_voxel = sc["idx"][:, a] == 5
        assert (slot[at_voxel] >= 0).any() == (extent[a] > 4)           # -voxel is the bound of an axis of 4
        assert (slot[~(sc["idx"] == 5).any(axis=1)] >= 0).all()


def test_minus_voxel_is_stored_on_every_axis_by_some_extent():
    assert all(any(e[a] > 4 for e in C.ANISO) for a in range(3))


# ---- the box rule --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("turns", (0, 1, 2))
@EXT_VOX
def test_box_bound_rows_sit_on_both_fp32_neighbours_of_the_bound(extent, voxel, turns):
    sc = C.box_bound(extent, voxel, turns)
    _check_model(sc)
    f = sc["frames"][0]
    w, t, rc = _world(f).astype(np.float64), f["W"][0][:3, 3], C.reach(extent, voxel)
    slot = C.model_end(sc)[1][0][0]
    assert np.array_equal(slot >= 0, sc["kind"] <= 1)
    seen = set()
    for i in np.flatnonzero(sc["axis"] >= 0):
        a, sg, k = sc["axis"][i], sc["sign"][i], sc["kind"][i]
        d = sg * (w[i, a] - t[a])
        w0 = np.float32(t[a] + sg * rc[a])
        assert float(w0) == t[a] + sg * rc[a]
        assert [None, d < rc[a], d == rc[a], d > rc[a]][k]
        assert np.float32(w[i, a]) == [None, np.nextafter(w0, np.float32(t[a])), w0, np.nextafter(w0, np.float32(sg * np.inf))][k]
        seen.add((a, sg, k))
    assert len(seen) == 18 and {0, 255, 256, 299} <= set(np.flatnonzero(sc["axis"] >= 0).tolist())
    assert (sc["kind"] == 1).sum() == 6 + 8                             # and the eight corners
    assert C.differs(sc, "box_le")
    assert not C.differs(dict(sc, frames=[dict(f, cloud=f["cloud"][:, sc["kind"] != 2], normals=f["normals"][:, sc["kind"] != 2])],
                              queries=None), "box_le")                  # only the rows ON the bound tell < from <=


# ---- ties ----------------------------------------------------------------------------------------------------------------------

@EXT_VOX
def test_ties_have_bit_equal_distances_and_the_first_candidate_in_order_wins(extent, voxel):
    sc = C.ties(extent, voxel)
    _check_model(sc)
    grids, slots, looks = C.model_end(sc)
    higher = lower = 0
    for s, g in enumerate(grids):
        a, b = sc["ab"][s]
        assert slots[0][s][a] >= 0 and slots[0][s][b] >= 0 and slots[0][s][2] >= 0 and slots[0][s][3] == -1, sc["names"][s]
        cand = C.tie_candidates(g, sc["queries"][s, 0])
        assert len(cand) == 3 and cand[0][0] == cand[1][0] < cand[2][0], sc["names"][s]        # bit-equal distances, a decoy
        cell, octant, dist = (v[0] for v in looks[s])
        assert (cell, octant) == (cand[0][5], cand[0][4]) == (slots[0][s][a] >> 3, slots[0][s][a] & 7), sc["names"][s]
        assert np.float32(dist).view(np.int32) == cand[0][0]
        if "cells" in sc["names"][s]:
            higher += cand[0][5] > cand[1][5]
            lower += cand[0][5] < cand[1][5]
        if "lower octant" in sc["names"][s]:
            assert cand[0][4] > cand[1][4]
    assert higher >= 3 and lower >= 3                                   # neither the lower nor the higher cell index always wins
    assert C.differs(sc, "tie_le")


# ---- the first point stays -----------------------------------------------------------------------------------------------------

@EXT_VOX
def test_first_point_stays_across_frames_and_the_lowest_row_within_one(extent, voxel):
    sc = C.first_point_stays(extent, voxel)
    _check_model(sc)
    frames = list((slot.copy(), [(g.keys.copy(), g.points.copy()) for g in grids]) for _, grids, slot, _ in C.model_frames(sc))
    for s in range(3):
        (slot0, state0), (slot1, state1) = frames
        keys0, pts0 = state0[s]
        keys1, pts1 = state1[s]
        assert (slot0[s] >= 0).all() and (slot1[s] >= 0).all()
        old = keys0 != vm.EMPTY
        assert np.array_equal(keys1[old], keys0[old]) and np.array_equal(pts1[old].view(np.int32), pts0[old].view(np.int32))
        lost = old[slot1[s] >> 3, slot1[s] & 7]                         # rows of frame 1 that aimed at an occupied octant
        assert lost.sum() > 20 and (~lost).sum() > 20
        new = (keys1 != vm.EMPTY) & ~old
        assert (keys1[new] >> 32 == 1).all() and (new.any(axis=1) & old.any(axis=1)).sum() > 10    # both kinds in one cell
        rows = C.DUPLICATES[s]
        assert len(set(slot0[s][list(rows)])) == 1
        sl = slot0[s][rows[0]]
        assert keys1[sl >> 3, sl & 7] == rows[0]                        # seq 0, the lowest row
        w = _world(sc["frames"][0], s)
        assert np.array_equal(pts1[sl >> 3, sl & 7], w[rows[0]]) and not np.array_equal(w[rows[0]], w[rows[1]])


# ---- begin ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extent", C.BEGIN_EXTENTS, ids=C.ext_id)
def test_begin_cases_hold_every_mask_combination_and_cut_inside_a_workgroup(extent):
    cells = extent[0] * extent[1] * extent[2]
    assert cells in (64, 4032, 4608, 16384)
    combos = set()
    for rnd in range(3):
        case = C.begin_case(extent, rnd)
        a, r, m = case["active"], case["restart"], case["armed"]
        combos |= set(zip((a != 0).tolist(), (r != 0).tolist(), (m != 0).tolist()))
        assert case["cleared"] == [bool(x and (y or z)) for x, y, z in zip(a, r, m)]
        assert np.array_equal(case["want"]["armed"], m)
        got, want = case["buffer"], case["want"]["buffer"]
        coord = want[:3 * cells * 8].view(np.int64).reshape(3, cells)
        assert np.array_equal(got[3 * cells * 8:], want[3 * cells * 8:])        # keys, points, normals stay, cleared or not
        for s in range(3):
            if case["cleared"][s]:
                assert (coord[s] == -1).all() and np.array_equal(case["want"]["P"][s], np.eye(4))
                assert case["want"]["nonempty"][s, 0] == 0 and case["want"]["seq"][s] == 0
            else:
                assert np.array_equal(coord[s], got[:3 * cells * 8].view(np.int64).reshape(3, cells)[s])
                assert np.array_equal(case["want"]["P"][s], case["P"][s]) and case["want"]["seq"][s] == 1000 + s
        assert (got[:3 * cells * 8].view(np.int64) != -1).all()                # the sentinel is not the empty word
    assert len(combos) == 8
    assert C.begin_case(extent, 2)["cleared"] == [False, False, True]          # armed on idle streams stays


# ---- pose and gates ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", C.GATE_S)
def test_gate_cases_mix_every_word(S):
    case = C.gate_case(S)
    words = set(zip((case["active"] != 0).tolist(), (case["insert"] != 0).tolist(), case["nonempty"][:, 0].tolist()))
    assert len(words) == min(S, 8) and (S == 1) == (words == {(True, True, 1)})
    assert S < 3 or set(case["armed"].tolist()) == {0, 1, -7}
    base = C.gate_model(case, C.GATE_CONFIGS[1])
    for cfg in C.GATE_CONFIGS:
        grids, slot, P, nonempty, seq, armed = C.gate_model(case, cfg)
        active = case["active"] != 0 if cfg["active"] else np.ones(S, bool)
        insert = active & (case["insert"] != 0 if cfg["insert"] else np.ones(S, bool))
        assert np.array_equal(armed[~active], case["armed"][~active]) and (armed[active] == 0).all()
        assert np.array_equal(seq, case["seq"] + 1 + insert) and np.array_equal(P[~active], case["P"][~active])
        assert np.array_equal(nonempty[:, 0], np.where(insert, 1, case["nonempty"][:, 0]))
        fresh = active & (case["nonempty"][:, 0] == 0)
        assert (P[fresh] == np.eye(4)).all()
        if slot is not None:
            assert ((slot >= 0).any(axis=1) == insert).all()
    assert S < 8 or not np.array_equal(base[2], C.gate_model(case, C.GATE_CONFIGS[0])[2])      # T given moves P


# ---- accumulate ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", C.ACC_N)
@EXT_VOX
def test_accumulate_cases_reach_every_bound_of_the_pair(extent, voxel, n):
    sc = C.accumulate_case(extent, voxel, n)
    g = C.model_end(sc)[0][0]
    assert sc["poison"] == (sorted({i for i in (0, 255, 256, 511, 512, n - 1) if i < n}) if n >= 255 else [])
    for name, (T, p) in sc["variants"].items():
        assert np.isnan(p[1]).all()
        pairs = []
        for md in C.max_dists(voxel):
            row, mag, (cell, octant, dist) = g.accumulate(p[0], np.eye(4) if T is None else T, C.SIGMA, md, P=sc["P"][0])
            pairs.append(row[model.PAIRS])
            assert (cell[sc["poison"]] == -1).all() and np.isinf(dist[sc["poison"]]).all()
            if name != "general":
                zero_n = (g.normals[np.maximum(cell, 0), np.maximum(octant, 0)] == 0).all(axis=1) & (cell >= 0)
                if md == 0.0:
                    assert row[model.PAIRS] == ((dist == 0) & ~zero_n).sum() >= 1
                if sc["zero_row"] is not None:
                    assert zero_n[sc["zero_row"]] and dist[sc["zero_row"]] == 0
        assert pairs[0] <= pairs[1] <= pairs[2] and (n < 255 or pairs[0] < pairs[1] < pairs[2] < n - len(sc["poison"]))
        if n >= 255:
            assert (dist[np.isfinite(dist)] > np.float32(voxel)).any()
