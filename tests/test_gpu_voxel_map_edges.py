"""The persistent voxel map at its coordinate edges on the GPU: the cases of tests/voxel_map_cases.py
through the stand-alone ops of ``voxel_map`` (begin, insert, pose, nearest, accumulate), bit for bit against the NumPy model of
tests/voxel_map_model.py -- slot and coordinate words, keys, stored points and normals, cell / octant / dist, P, seq,
nonempty and armed -- and the sums against its fp64 row within 1e-12 sum |term| with the pair count exact.  Every case runs
twice and must give the same bits.  tests/test_voxel_map_cases_cpu.py proves that every case reaches the edge it names."""
import copy

import numpy as np
import pytest
import torch

import icp_model as model
import voxel_map_cases as C
from pwclonet_pylidarslam_amd import _lib, voxel_map

pytestmark = pytest.mark.gpu

EXT_VOX = pytest.mark.parametrize("extent, voxel", list(zip(C.ANISO, C.VOXELS)) + [(C.ANISO[0], 2.0)],
                                  ids=lambda v: C.ext_id(v) if isinstance(v, tuple) else str(v))


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize])


def _grid_is(sec, s, g):
    """A device grid's stream s holds the model grid's bits, section by section."""
    ok = np.array_equal(sec["coord"][s].cpu().numpy(), g.coord) and np.array_equal(sec["keys"][s].cpu().numpy(), g.keys)
    for name, want in (("points", g.points), ("normals", g.normals)):
        ok = ok and np.array_equal(sec[name][s].cpu().numpy().view(np.int32), want.view(np.int32))
    return ok


def _model(sc):
    """The model's side of a scenario, computed once for both runs: per frame (slot, copies of the grids), and the lookups."""
    frames = [(slot, copy.deepcopy(grids)) for _, grids, slot, _ in C.model_frames(sc)]
    looks = None if sc["queries"] is None else [g.lookup(sc["queries"][s]) for s, g in enumerate(frames[-1][1])]
    return frames, looks


def _run(dev, sc, want_frames, looks):
    """Insert the scenario's frames (each followed by the pose launch), look its queries up; every frame against the model.
    -> the tensors a second run must repeat."""
    extent, voxel = sc["extent"], sc["voxel"]
    S = sc["frames"][0]["cloud"].shape[0]
    grid = voxel_map.new_grid(S, extent, dev)
    sec = voxel_map.sections(grid, S, extent)
    P = torch.zeros((S, 4, 4), dtype=torch.float64, device=dev)
    nonempty = torch.zeros((S, 1), dtype=torch.int32, device=dev)
    seq = torch.zeros((S,), dtype=torch.int32, device=dev)
    out = [grid]
    for k, ((want, grids), f) in enumerate(zip(want_frames, sc["frames"])):
        P.copy_(_dev(f["W"], dev))
        slot = voxel_map.insert(grid, extent, voxel, _dev(f["cloud"], dev), _dev(f["normals"], dev), P, seq)
        voxel_map.pose(P, nonempty, seq)
        assert np.array_equal(slot.cpu().numpy(), want), (sc["edge"], k)
        for s, g in enumerate(grids):
            assert _grid_is(sec, s, g), (sc["edge"], k, s)
        assert seq.tolist() == [k + 1] * S and nonempty[:, 0].tolist() == [1] * S
        want_P = f["W"] if k else np.stack([np.eye(4)] * S)             # the pose launch: I where the map was empty, else P
        assert np.array_equal(_bits(P.cpu().numpy()), _bits(want_P))
        out.append(slot)
    if sc["queries"] is not None:
        eye = torch.eye(4, dtype=torch.float64, device=dev).expand(S, 4, 4).contiguous()
        cell, octant, dist = voxel_map.nearest(grid, extent, voxel, _dev(sc["queries"], dev), eye)
        for s, (wc, wo, wd) in enumerate(looks):
            assert np.array_equal(cell[s].cpu().numpy(), wc) and np.array_equal(octant[s].cpu().numpy(), wo), (sc["edge"], s)
            assert np.array_equal(_bits(dist[s].cpu().numpy()), _bits(wd)), (sc["edge"], s)
        out += [cell, octant, dist]
    return out


def _twice(dev, sc):
    want = _model(sc)
    a, b = _run(dev, sc, *want), _run(dev, sc, *want)
    assert len(a) == len(b) and all(torch.equal(x.view(torch.uint8) if x.dtype == torch.float32 else x,
                                                y.view(torch.uint8) if y.dtype == torch.float32 else y) for x, y in zip(a, b))
    _lib.synchronize(dev)
    return a


# ---- insertion and lookup ------------------------------------------------------------------------------------------------------

@EXT_VOX
def test_anisotropic_walk(cuda, extent, voxel):
    _twice(cuda, C.aniso_walk(extent, voxel))


@pytest.mark.parametrize("direction", list(C.DIRECTIONS))
@EXT_VOX
def test_wrap_on_every_axis_in_both_directions(cuda, extent, voxel, direction):
    _twice(cuda, C.wrap_walk(extent, voxel, direction))


@pytest.mark.parametrize("end", ("low", "high"))
@pytest.mark.parametrize("axes", ((0, 1, 2), (0,), (1,), (2,)), ids=("corner", "x", "y", "z"))
@EXT_VOX
def test_range_ends(cuda, extent, voxel, axes, end):
    sc = C.range_end(extent, voxel, end, axes)
    out = _twice(cuda, sc)
    assert np.array_equal(out[1][0].cpu().numpy() >= 0, sc["stored"])   # the half indices beyond the end: slot -1
    n = len(sc["stored"])
    assert (out[-3][0, 2 * n:] == -1).all()                             # the opposite end: a neighbour out of range is skipped


@EXT_VOX
def test_rows_around_zero(cuda, extent, voxel):
    _twice(cuda, C.zero_straddle(extent, voxel))


@pytest.mark.parametrize("turns", (0, 1, 2))
@EXT_VOX
def test_box_rule_at_its_bound(cuda, extent, voxel, turns):
    sc = C.box_bound(extent, voxel, turns)
    out = _twice(cuda, sc)
    assert np.array_equal(out[1][0].cpu().numpy() >= 0, sc["kind"] <= 1)         # the inner neighbour is stored, the bound is not


@EXT_VOX
def test_exact_ties_keep_the_first_candidate(cuda, extent, voxel):
    sc = C.ties(extent, voxel)
    out = _twice(cuda, sc)
    slot, cell, octant = out[1].cpu().numpy(), out[-3].cpu().numpy(), out[-2].cpu().numpy()
    for s, (a, b) in enumerate(sc["ab"]):
        assert cell[s, 0] * 8 + octant[s, 0] == slot[s, a] != slot[s, b], sc["names"][s]


@EXT_VOX
def test_first_point_stays(cuda, extent, voxel):
    _twice(cuda, C.first_point_stays(extent, voxel))


# ---- begin -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extent", C.BEGIN_EXTENTS, ids=C.ext_id)
def test_begin_against_the_model_byte_for_byte(cuda, extent):
    for rnd in range(len(C.BEGIN_ROUNDS)):
        case = C.begin_case(extent, rnd)
        runs = []
        for _ in range(2):
            t = {k: _dev(case[k], cuda) for k in ("buffer", "P", "nonempty", "seq", "active", "restart", "armed")}
            voxel_map.begin(t["buffer"], extent, t["P"], t["nonempty"], t["seq"], active=t["active"], restart=t["restart"],
                            armed=t["armed"])
            for k, want in case["want"].items():
                assert np.array_equal(_bits(t[k].cpu().numpy()), _bits(want)), (case["edge"], k)
            assert np.array_equal(t["active"].cpu().numpy(), case["active"])
            assert np.array_equal(t["restart"].cpu().numpy(), case["restart"])
            runs.append(t)
        assert all(torch.equal(runs[0][k].view(torch.uint8), runs[1][k].view(torch.uint8)) for k in runs[0])
    if extent == C.BEGIN_EXTENTS[0]:                                    # no masks at all: every stream keeps its map
        t = {k: _dev(case[k], cuda) for k in ("buffer", "P", "nonempty", "seq")}
        voxel_map.begin(t["buffer"], extent, t["P"], t["nonempty"], t["seq"])
        assert all(np.array_equal(_bits(t[k].cpu().numpy()), _bits(case[k])) for k in t)
    _lib.synchronize(cuda)


# ---- pose and gates ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", C.GATE_S)
def test_pose_and_gates(cuda, S):
    case = C.gate_case(S)
    extent, voxel = case["extent"], case["voxel"]
    for cfg in C.GATE_CONFIGS:
        grids, want_slot, want_P, want_nonempty, want_seq, want_armed = C.gate_model(case, cfg)
        runs = []
        for _ in range(2):
            P, nonempty, seq, armed = (_dev(case[k], cuda) for k in ("P", "nonempty", "seq", "armed"))
            T = _dev(case["T"], cuda) if cfg["T"] else None
            active = _dev(case["active"], cuda) if cfg["active"] else None
            insert = _dev(case["insert"], cuda) if cfg["insert"] else None
            out = []
            if case["with_grid"]:
                grid = voxel_map.new_grid(S, extent, cuda)
                pre, frame = case["prefill"], case["frame"]
                voxel_map.insert(grid, extent, voxel, _dev(pre["cloud"], cuda), _dev(pre["normals"], cuda), P, seq)
                seq += 1
                slot = voxel_map.insert(grid, extent, voxel, _dev(frame["cloud"], cuda), _dev(frame["normals"], cuda), P, seq,
                                        T=T, nonempty=nonempty if cfg["nonempty"] else None, active=active, insert=insert)
                assert np.array_equal(slot.cpu().numpy(), want_slot), (S, cfg)
                out += [grid, slot]
            else:
                seq += 1
            voxel_map.pose(P, nonempty, seq, T=T, armed=armed, active=active, insert=insert)
            if case["with_grid"]:
                sec = voxel_map.sections(grid, S, extent)
                for s, g in enumerate(grids):
                    assert _grid_is(sec, s, g), (S, cfg, s)
            assert np.array_equal(_bits(P.cpu().numpy()), _bits(want_P)), (S, cfg)
            assert np.array_equal(nonempty.cpu().numpy(), want_nonempty) and np.array_equal(seq.cpu().numpy(), want_seq)
            assert np.array_equal(armed.cpu().numpy(), want_armed), (S, cfg)
            runs.append(out + [P, nonempty, seq, armed])
        assert all(torch.equal(a, b) for a, b in zip(*runs))
    _lib.synchronize(cuda)


# ---- accumulate --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", C.ACC_N)
@EXT_VOX
def test_accumulate_shapes_and_bounds(cuda, extent, voxel, n):
    sc = C.accumulate_case(extent, voxel, n)
    want = _model(sc)
    grid, g = _run(cuda, sc, *want)[0], want[0][-1][1][0]
    P, active = _dev(sc["P"], cuda), _dev(sc["active"], cuda)
    for name, (T, p) in sc["variants"].items():
        Td = None if T is None else _dev(np.stack([T, T]), cuda)
        for md in C.max_dists(voxel):
            row, mag, near = g.accumulate(p[0], np.eye(4) if T is None else T, C.SIGMA, md, P=sc["P"][0])
            runs = []
            for _ in range(2):
                partial, cell, octant, dist = voxel_map.accumulate(grid, extent, voxel, _dev(p, cuda), P, Td, sigma=C.SIGMA,
                                                                   max_dist=md, active=active, nearest=True)
                runs.append((partial, cell, octant, dist))
            assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(*runs))
            got = partial[0].cpu().numpy().sum(axis=0)
            print("%s n=%d T=%s max_dist=%g: pairs %d (model %d), worst |diff| / sum|term| %.2e"
                  % (C.ext_id(extent), n, name, md, got[model.PAIRS], row[model.PAIRS],
                     (np.abs(got - row) / np.maximum(mag, 1e-300)).max()))
            assert np.array_equal(cell[0].cpu().numpy(), near[0]) and np.array_equal(octant[0].cpu().numpy(), near[1])
            assert np.array_equal(_bits(dist[0].cpu().numpy()), _bits(near[2])), (name, md)
            assert got[model.PAIRS] == row[model.PAIRS] and (np.abs(got - row) <= 1e-12 * mag + 1e-300).all(), (name, md)
            assert (_bits(partial[1].cpu().numpy()) == 0).all()         # the idle stream with a NaN cloud: exact zeros
            assert (cell[1] == -1).all() and (octant[1] == -1).all() and torch.isinf(dist[1]).all()
    _lib.synchronize(cuda)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def test_refused_arguments_raise_before_any_launch(cuda):
    extent, voxel, S, n = (6, 4, 10), 1.0, 2, 8
    grid = voxel_map.new_grid(S, extent, cuda)
    p = torch.zeros((S, n, 3), dtype=torch.float32, device=cuda)
    P = torch.eye(4, dtype=torch.float64, device=cuda).expand(S, 4, 4).contiguous()
    nonempty = torch.zeros((S, 1), dtype=torch.int32, device=cuda)
    seq = torch.zeros((S,), dtype=torch.int32, device=cuda)
    calls, real = [], _lib.call
    _lib.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        for bad in ((6, 5, 10), (6, 4, 2), (6, 4), (6, 4, 1026), (6.5, 4, 10)):
            for op in (lambda e: voxel_map.begin(grid, e, P, nonempty, seq),
                       lambda e: voxel_map.insert(grid, e, voxel, p, p.clone(), P, seq),
                       lambda e: voxel_map.accumulate(grid, e, voxel, p, P), lambda e: voxel_map.nearest(grid, e, voxel, p, P)):
                with pytest.raises(ValueError, match="extent"):
                    op(bad)
        for md in (np.nextafter(1.0, 2.0), 1.5, -0.25, float("nan")):
            with pytest.raises(ValueError, match="max_dist"):
                voxel_map.accumulate(grid, extent, voxel, p, P, max_dist=md)
        big = torch.zeros((1025, 4, 4), dtype=torch.float64, device=cuda)
        with pytest.raises(ValueError, match="S=1025"):
            voxel_map.pose(big, torch.zeros((1025, 1), dtype=torch.int32, device=cuda),
                           torch.zeros((1025,), dtype=torch.int32, device=cuda))
        with pytest.raises(ValueError, match="grid"):
            voxel_map.insert(grid[:-8], extent, voxel, p, p.clone(), P, seq)
        with pytest.raises(ValueError, match="active"):
            voxel_map.insert(grid, extent, voxel, p, p.clone(), P, seq, active=torch.ones(S + 1, dtype=torch.int32, device=cuda))
        assert calls == []                                              # the Python layer refused all of these itself
    finally:
        _lib.call = real
    # the library's own refusals: an error return, no launch.  Python cannot pass `cell` without `octant`; the C entry can.
    partial = torch.full((S, 1, 32), 7.0, dtype=torch.float64, device=cuda)
    cell = torch.full((S, n), 5, dtype=torch.int32, device=cuda)
    ptr = lambda t: t.data_ptr()
    with pytest.raises(RuntimeError, match="cell, octant and dist come together"):
        _lib.call("voxel_accumulate_kernel_wrapper", cuda, S, n, *extent, voxel, ptr(p), ptr(P), 0, ptr(grid), 0.5, 1.0,
                  ptr(partial), ptr(cell), 0, 0, 0)
    with pytest.raises(RuntimeError, match="max_dist"):
        _lib.call("voxel_accumulate_kernel_wrapper", cuda, S, n, *extent, voxel, ptr(p), ptr(P), 0, ptr(grid), 0.5, 1.5,
                  ptr(partial), 0, 0, 0, 0)
    with pytest.raises(RuntimeError, match="extent"):
        _lib.call("voxel_accumulate_kernel_wrapper", cuda, S, n, 6, 5, 10, voxel, ptr(p), ptr(P), 0, ptr(grid), 0.5, 1.0,
                  ptr(partial), 0, 0, 0, 0)
    with pytest.raises(RuntimeError, match="extent"):
        _lib.call("voxel_insert_kernel_wrapper", cuda, S, n, 6, 4, 2, voxel, ptr(p), ptr(p), ptr(P), 0, 0, ptr(seq), ptr(grid),
                  ptr(cell), 0, 0)
    with pytest.raises(RuntimeError, match="S=1025"):
        _lib.call("voxel_pose_kernel_wrapper", cuda, 1025, 0, ptr(big), ptr(big), ptr(big), 0, 0, 0)
    _lib.synchronize(cuda)
    assert (partial == 7.0).all() and (cell == 5).all() and not big.any()          # nothing ran
    assert torch.equal(grid, voxel_map.new_grid(S, extent, cuda))
