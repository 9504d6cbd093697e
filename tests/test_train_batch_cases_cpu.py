"""tests/train_batch_cases.py and the additions to tests/train_batch_model.py on the CPU: the committed Philox collisions are
real, every table of tests/test_gpu_train_batch_edges.py reaches what it names (read off the model and off the ``per_wave``
formula of DESIGN.md section 13), the model's two statements of the subset rule agree on all of them, and every planted fault
of the model changes the expected output of the table that is there to catch it.

Run with ``-s`` for the figures."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_batch_cases as TC                                                   # noqa: E402
import train_batch_model as model                                                # noqa: E402

_EXPECTED = {}


def _arrays_and_expected(case):
    if case["name"] not in _EXPECTED:
        arrays = TC.materialise(case)
        aug = None
        if case["mode"] == 1:                                                    # what the device would draw, once
            aug = np.stack([model.draw_aug(b, case["step"], case["seed"]) for b in range(len(case["lengths"]))])
        _EXPECTED[case["name"]] = (arrays, TC.expected(case, arrays, aug=aug), aug)
    return _EXPECTED[case["name"]]


def _differs(a, b):
    return any(not np.array_equal(a[k].view(np.int32) if a[k].dtype == np.float32 else a[k],
                                  b[k].view(np.int32) if b[k].dtype == np.float32 else b[k])
               for k in ("indices", "counts", "xyz_f1", "xyz_f2", "gt"))


def _clamped_n(case, b):
    R = case["R"]
    return min(min(max(v, 0), R) for v in case["lengths"][b])


def test_case_names_are_unique_and_tables_complete():
    names = [c["name"] for c in TC.all_cases()]
    assert len(names) == len(set(names))
    tables = {c["table"] for c in TC.all_cases()}
    assert tables == {"padding", "counts", "row_edges", "device_lengths", "ties", "quat", "euler", "wide"}
    for table in ("padding", "counts", "row_edges", "device_lengths"):
        assert {c["dataset"] for c in TC.all_cases() if c["table"] == table} == set(TC.DATASETS), table
    assert {(c["dataset"], c["mode"]) for c in TC.pose_cases()} == {(d, m) for d in TC.DATASETS for m in (0, 2)}


def test_collision_constants_are_real():
    per_wave, ranges = model.wave_layout(TC.TIE_R)
    assert per_wave == 16384 and ranges[15] == (15 * 16384, TC.TIE_R)
    for key, c in TC.COLLISIONS.items():
        i, j = c["rows"]
        w = model.words(np.array([i, j]), c["cloud"], c["step"], model.SELECT, c["seed"])
        assert i < j < TC.TIE_R and int(w[0]) == int(w[1]) == c["word"], key
    (i, j), (k, l) = TC.COLLISIONS["cross"]["rows"], TC.COLLISIONS["same"]["rows"]
    assert i // per_wave != j // per_wave
    assert k // per_wave == l // per_wave and k // 64 != l // 64
    # the search that found them, for the dense triple: the pair is there, with its rank, and qualifies (rank < 8192)
    c = TC.COLLISIONS["dense"]
    found = TC.find_collisions(c["seed"], c["step"], c["cloud"])
    print("\n%d colliding pairs at seed %d step %d cloud %d" % (len(found), c["seed"], c["step"], c["cloud"]))
    assert dict(rows=c["rows"], word=c["word"], rank=c["rank"]) in found and c["rank"] < 8192
    assert all(f["rows"][1] - f["rows"][0] >= 64 for f in found)                # none inside one 64-row step


@pytest.mark.parametrize("case", TC.selection_cases(), ids=lambda c: c["name"])
def test_rows_survive_by_construction_and_both_rules_agree(case):
    """``model.filter_rows`` keeps exactly the rows the case says, in both frames; wherever the subset branch runs, the
    stable (word, row) selection gives the rows the 64-bit keys give."""
    arrays, ref, _aug = _arrays_and_expected(case)
    subset = 0
    for b in range(len(case["lengths"])):
        n = _clamped_n(case, b)
        for f in range(2):
            _xyz, keep = model.filter_rows(case["dataset"], arrays["sweeps"][b, f], arrays["tr"])
            assert np.array_equal(keep, arrays["keep"][b, f]), (b, f)
            count = int(keep[:n].sum())
            assert ref["counts"][2 * b + f] == count
            if n and count >= case["npoints"]:
                subset += 1
                rows = model.select_rows_stable(keep[:n], case["npoints"], 2 * b + f, case["step"], case["seed"])
                assert np.array_equal(rows, ref["indices"][2 * b + f]), (b, f)
                assert len(set(rows.tolist())) == case["npoints"]
    assert subset or case["table"] == "device_lengths" or case["table"] == "counts"
    if case["table"] in ("counts", "device_lengths"):
        assert subset >= 2


def test_padding_table():
    """P, the power of two the launcher picks (at least 2), exceeds npoints in every case but npoints = 2; enough survivors
    for the subset branch; n no multiple of 64."""
    assert {c["npoints"] for c in TC.padding_cases()} == set(TC.PADDING_NPOINTS)
    for case in TC.padding_cases():
        m = case["npoints"]
        P = 2
        while P < m:
            P *= 2
        assert P > m or m == 2
        _arrays, ref, _aug = _arrays_and_expected(case)
        assert case["R"] % 64 and (ref["counts"] >= m).all() and (ref["counts"] <= 3 * m).all()


def test_count_table():
    for case in TC.count_cases():
        m = case["npoints"]
        _arrays, ref, _aug = _arrays_and_expected(case)
        assert ref["counts"].tolist() == [c for c in (0, 1, m - 1, m, m + 1) for _f in range(2)]
        assert ref["indices"].min() >= 0                                         # n > 0 everywhere: count 0 draws over the rows


def test_row_edge_table():
    """The non-empty wave ranges from the per_wave formula itself, not from the model."""
    for n, waves in TC.ROW_EDGE_WAVES.items():
        per_wave = ((n + 15) // 16 + 63) // 64 * 64
        nonempty = [w for w in range(16) if w * per_wave < min(n, w * per_wave + per_wave)]
        assert nonempty == list(range(waves)), n
    assert ((1024 + 15) // 16 + 63) // 64 * 64 == 64 and ((1025 + 15) // 16 + 63) // 64 * 64 == 128
    for case in TC.row_edge_cases():
        arrays, ref, _aug = _arrays_and_expected(case)
        assert [min(v) for v in case["lengths"]] == case["n"] and case["n"][:8] == list(TC.ROW_EDGE_N)
        per_wave = ((4096 + 15) // 16 + 63) // 64 * 64
        for b, wave in ((8, 0), (9, 15)):
            rows = np.nonzero(arrays["keep"][b, 0])[0]
            assert set((rows // per_wave).tolist()) == {wave} and len(rows) >= case["npoints"]
        assert ref["counts"][0] == 1 and (ref["counts"][2:] >= case["npoints"]).all()     # n = 1: one survivor, drawn 16 times


def test_device_length_table():
    for case in TC.device_length_cases():
        R = case["R"]
        assert case["device_lengths"] and [_clamped_n(case, b) for b in range(5)] == case["n"] == [0, 0, R, 7, 150]
        assert case["lengths"][:4] == [[0, 5], [-3, 7], [R + 9, R + 1], [7, R]]
        _arrays, ref, _aug = _arrays_and_expected(case)
        assert (ref["indices"][:4] == -1).all() and (ref["counts"][:4] == 0).all()
        for x in (ref["xyz_f1"], ref["xyz_f2"]):
            assert not x[:2].view(np.int32).any()                                # +0.0 words, also in the moved cloud
        assert ref["counts"][5] == 0 and ref["indices"][5].max() > R // 2 and ref["indices"][5].max() < R
        assert 0 < ref["counts"][6] < case["npoints"] and ref["counts"][8] >= case["npoints"]
    # the argument is explicit: without it the model takes the lengths as they are, as before
    rows, count = model.select_rows(np.zeros(0, dtype=bool), 4, 0, 0, 1)
    assert rows.tolist() == [-1] * 4 and count == 0


def test_tie_table():
    """``ties`` and ``need`` as the radix select would find them, on the cloud that holds the collision; the named rows are
    in, respectively out of, the model's selection; in the selection both tied rows are neighbours in row order."""
    names = [c["name"] for c in TC.tie_cases()]
    assert sum("kitti360" not in n for n in names) == 2 and len(names) == 9
    for case in TC.tie_cases():
        c = TC.COLLISIONS[case["key"]]
        arrays, ref, _aug = _arrays_and_expected(case)
        cloud = c["cloud"]
        info = model.select_info(arrays["keep"][0, cloud], case["npoints"], cloud, case["step"], case["seed"])
        assert (info["ties"], info["need"]) == (case["ties"], case["need"]), (case["name"], info)
        got = ref["indices"][cloud].tolist()
        assert all(r in got for r in case["take"]) and not any(r in got for r in case["leave"]), case["name"]
        if case["ties"] == 2:
            assert info["threshold"] == c["word"]
            if case["need"] == 2:
                assert got[-2:] == list(c["rows"])                               # the last two, in row order
            else:
                assert got[-1] == c["rows"][0]
        else:
            assert info["threshold"] != c["word"]
        if case["key"] != "dense":                                               # a smaller-word survivor lies behind the pair
            w = model.words(np.arange(TC.TIE_R), cloud, c["step"], model.SELECT, c["seed"])
            surv = np.nonzero(arrays["keep"][0, cloud])[0]
            assert len(surv) == 12 and (w[surv] < c["word"]).sum() == 5 and (w[surv] > c["word"]).sum() == 5
            assert surv[w[surv] < c["word"]].max() > c["rows"][1]
        other = 1 - cloud                                                        # the other frame: same rows, no tie there
        assert model.select_info(arrays["keep"][0, other], case["npoints"], other, case["step"], case["seed"])["ties"] == 1


def test_quaternion_table():
    assert {x for _n, _r, x in TC.QUAT_ROTATIONS} == {0, 1, 2, 3}
    for name, R, branch in TC.QUAT_ROTATIONS:
        assert model.quat_branch(R) == branch, name
        assert np.abs(R.dot(R.T) - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1) < 1e-15, name
        dec = [R[0, 0], R[1, 1], R[2, 2], (R[0, 0] + R[1, 1]) + R[2, 2]]
        top = sorted(dec)[-2:]
        if name in TC.QUAT_TIES:
            assert top[0] == top[1] and model.quat_branch(R, "quat_ge") == 3, name       # exact, and the last maximum differs
        else:
            assert top[1] - top[0] > 0.1, name
    want = {"third_turn": [0.5, 0.5, 0.5, 0.5], "third_turn_back": [-0.5, 0.5, 0.5, 0.5]}
    for name, R, _branch in TC.QUAT_ROTATIONS:
        if name in want:
            assert model.quat_diag(R).tolist() == want[name]                     # the m00 form's sign: x > 0


def test_euler_table():
    seen = set()
    for name, R, gimbal in TC.EULER_ROTATIONS:
        c = np.sqrt(R[2, 2] * R[2, 2] + R[1, 2] * R[1, 2])
        print("\n%-16s c = %.17g (4 eps = %.17g)" % (name, c, TC.EPS4))
        assert (not c > TC.EPS4) == gimbal, name
        seen.add(gimbal)
        assert not np.signbit(R).any() or (R[np.signbit(R)] != 0).all()          # no -0.0 entry
    R = dict((n, r) for n, r, _g in TC.EULER_ROTATIONS)
    assert seen == {True, False}
    assert R["pitch_up"].tolist() == [[0, 0, 1], [0, 1, 0], [-1, 0, 0]]
    assert R["pitch_down"].tolist() == [[0, 0, -1], [0, 1, 0], [1, 0, 0]]
    c = lambda r: np.sqrt(r[2, 2] * r[2, 2] + r[1, 2] * r[1, 2])
    assert c(R["pitch_up"]) == 0 and c(R["edge_at"]) == TC.EPS4 and c(R["edge_above"]) == np.nextafter(TC.EPS4, 1.0)
    assert TC.EPS4 < c(R["delta_above"]) < 1.2 * TC.EPS4 and 0.8 * TC.EPS4 < c(R["delta_below"]) < TC.EPS4


def test_wide_table():
    for case in TC.wide_cases():
        assert len(case["lengths"]) == 257
    p = TC.given_params(257)
    assert p.dtype == np.float32 and (np.abs(p) <= np.float32(model.AUG_CLIP)).all()
    assert len({tuple(r) for r in p.tolist()}) == 257


@pytest.mark.parametrize("case", [c for c in TC.pose_cases() + TC.wide_cases() if c["mode"] == 2], ids=lambda c: c["name"])
def test_composed_poses_are_away_from_every_discontinuity(case):
    """Mode 2 composes the tables' rotations with an augmentation, which moves them off the exact ties.  The model is only
    a reference where its output is continuous: a relative change of 1e-13 of T_diff (far above what the two fp64
    evaluations differ by, 1e-12 is the bound on T_gt) moves no quaternion by more than 1e-9."""
    arrays, ref, _aug = _arrays_and_expected(case)
    worst = 0.0
    for sign in (1.0, -1.0):
        moved = dict(arrays)
        k = np.arange(arrays["t_diff"].size).reshape(arrays["t_diff"].shape)
        moved["t_diff"] = arrays["t_diff"] * (1.0 + sign * 1e-13 * ((k * 7) % 5 - 2))
        gt = np.stack([model.pose(case["dataset"], moved["t_diff"][b], arrays["aug"][b])[2] for b in range(len(case["lengths"]))])
        worst = max(worst, np.abs(gt[:, 3:].astype(np.float64) - ref["gt"][:, 3:]).max())
    print("\n%s: quaternion moves by at most %.2e" % (case["name"], worst))
    assert worst <= 2.0 ** -23


FAULT_TABLE = {"tie_high_row": "ties", "tie_all": "ties", "tie_none": "ties", "count_gt": "counts", "no_clamp": "device_lengths",
               "n0_row0": "device_lengths", "quat_ge": "quat", "no_gimbal": "euler", "sort_pow2": "padding"}


@pytest.mark.parametrize("fault", model.FAULTS)
def test_every_fault_is_caught(fault):
    """Each planted fault changes the expected output of at least one case of the table that is there for it; for the tie
    faults both regimes (sparse and dense, KITTI-360 and KITTI) catch it."""
    assert set(FAULT_TABLE) == set(model.FAULTS)
    caught = []
    for case in TC.all_cases():
        if case["table"] != FAULT_TABLE[fault] or (case["table"] in ("quat", "euler") and case["mode"] != 0):
            continue
        arrays, ref, aug = _arrays_and_expected(case)
        if _differs(ref, TC.expected(case, arrays, aug=aug, fault=fault)):
            caught.append(case["name"])
    print("\n%s: caught by %s" % (fault, caught))
    assert caught, fault
    if fault.startswith("tie_"):
        for must in ("ties-cross_one_of_two-kitti360", "ties-cross_one_of_two-kitti", "ties-same_one_of_two-kitti360",
                     "ties-dense_one_of_two-kitti360", "ties-dense_one_of_two-kitti"):
            assert must in caught, (fault, must)
        if fault != "tie_none":                                                  # (it drops the threshold row of every case)
            assert "ties-cross_below-kitti360" not in caught and "ties-cross_above-kitti360" not in caught
    if fault == "count_gt":
        assert len(caught) == 4                                                  # both npoints, both row bodies
    if fault == "sort_pow2":                                                     # every npoints that is no power of two
        assert len(caught) == 2 * sum(m & (m - 1) != 0 for m in TC.PADDING_NPOINTS)
    if fault == "quat_ge":
        assert caught == ["quat-mode0-kitti360"]
    if fault == "no_gimbal":
        assert caught == ["euler-mode0-kitti"]
    if fault in ("no_clamp", "n0_row0"):
        assert len(caught) == 2
