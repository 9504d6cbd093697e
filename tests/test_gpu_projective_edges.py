"""The projective registration at its edges on the GPU: the cases of tests/projective_cases.py through
``projective.vertex_map``, ``normal_map``, ``model_build``, ``accumulate`` and ``map_push``, against the NumPy model of
tests/projective_model.py.  tests/test_projective_cases_cpu.py proves that every case reaches the edge it names and tells
the model from the fault that edge is about.

The exact-argument cases rest on atan2f / asinf returning 0, +-pi/2 and +-pi at arguments on the axes; every other point is
>= 1e-3 px from a rounding boundary.  Normals are held to one fp32 rounding of a unit component (2^-24) plus the fp64
uncertainty of the solve, measured per case as the disagreement of the model's LU solve with the adjugate formula."""
import numpy as np
import pytest
import torch

import icp_model as icp
import projective_cases as C
import projective_model as model
from pwclonet_pylidarslam_amd import _lib, projective, registration

pytestmark = pytest.mark.gpu

F = np.float32


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _ids(cases):
    return [c["edge"] for c in cases]


# ---- vertex map ----------------------------------------------------------------------------------------------------------------

VERTEX = C.vertex_cases()


@pytest.mark.parametrize("c", VERTEX, ids=_ids(VERTEX))
def test_vertex_map(cuda, c):
    S = c["points"].shape[0]
    kw = dict(height=c["H"], width=c["W"], **c["fov"])
    runs = []
    for _ in range(2):
        vmap, rows = projective.vertex_map(_dev(c["points"], cuda), lengths=_dev(c["lengths"], cuda), keep=_dev(c["keep"], cuda),
                                           **kw)
        runs.append((vmap.cpu().numpy(), rows.cpu().numpy()))
    for s in range(S):
        want_v, want_r = model.vertex_map(c["points"][s], c["im"], None if c["lengths"] is None else c["lengths"][s],
                                          None if c["keep"] is None else c["keep"][s])
        assert np.array_equal(runs[0][1][s], want_r), (c["edge"], s, runs[0][1][s], want_r)
        assert _same(runs[0][0][s], want_v), (c["edge"], s)
    for (s, y, x), i in c["wins"].items():
        assert runs[0][1][s, y, x] == i
    assert _same(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])         # two runs: the same bits


# ---- normal map ----------------------------------------------------------------------------------------------------------------

def _normals(cuda, vmaps, k):
    return projective.normal_map(_dev(np.stack(vmaps), cuda), kernel_size=k).cpu().numpy()


def _check_normals(got, vmap, k, what):
    """Pattern equal to the model's; components within 2^-24 + the measured fp64 uncertainty; unit length; away from the sensor."""
    with np.errstate(all="ignore"):
        n, _ = model.normal_map(vmap, k)
    nz = (n != 0).any(axis=-1)
    assert np.array_equal(nz, (got != 0).any(axis=-1)), what
    if nz.any():
        bound = C.HALF_ULP + C.solve_disagreement(vmap, k)
        err = np.abs(got[nz].astype(np.float64) - n[nz]).max()
        print("%s k=%d: worst component error %.3e (bound %.3e)" % (what, k, err, bound))
        assert err <= bound, what
        assert np.abs(np.linalg.norm(got[nz].astype(np.float64), axis=-1) - 1.0).max() < 1e-6
        assert ((got[nz] * vmap[nz]).sum(axis=-1) > 0).all()
    return nz


@pytest.mark.parametrize("k", (3, 5))
@pytest.mark.parametrize("H, W", C.NORMAL_SHAPES)
def test_normal_map_random_occupancy(cuda, H, W, k):
    c = C.occupancy(H, W)
    got = _normals(cuda, [c["vmap"], c["vmap"]], k)
    _check_normals(got[0], c["vmap"], k, c["edge"])
    assert _same(got[0], got[1])


@pytest.mark.parametrize("k", (3, 5))
def test_normal_map_planes_and_the_determinant_cut(cuda, k):
    cases = [C.plane(w) for w in ("far", "near", "cut")]
    got = _normals(cuda, [c["vmap"] for c in cases], k)
    for c, g in zip(cases[:2], got):
        nz = _check_normals(g, c["vmap"], k, c["edge"])
        assert np.array_equal(nz, c["hit"])                             # far above the cut: every hit pixel
    assert not got[2].any()                                             # far below it: none


@pytest.mark.parametrize("k", (3, 5))
def test_normal_map_lonely_pixels_and_nan(cuda, k):
    lone, bad = C.lonely(), C.nan_vertex()
    got = _normals(cuda, [lone["vmap"], bad["vmap"], bad["emptied"]], k)
    _check_normals(got[0], lone["vmap"], k, lone["edge"])
    for at in (lone["empty"], lone["alone"]) + lone["pair"] + lone["column"]:
        assert not got[0][at].any()
    for at in lone["triple"]:
        assert got[0][at].any()
    _check_normals(got[2], bad["emptied"], k, bad["edge"])
    h, (y, x) = k // 2, bad["at"]
    yy, xx = np.meshgrid(np.arange(bad["H"]), np.arange(bad["W"]), indexing="ij")
    inside = (np.abs(yy - y) <= h) & (np.abs(xx - x) <= h)
    assert not got[1][inside].any()                                     # every window that holds the NaN
    assert _same(got[1][~inside], got[2][~inside])                      # and no other


# ---- model build ---------------------------------------------------------------------------------------------------------------

BUILD = C.build_cases()


@pytest.mark.parametrize("c", BUILD, ids=_ids(BUILD))
def test_model_build(cuda, c):
    S, M = c["live"].shape
    ws = torch.zeros((_lib.load().proj_model_build_workspace_bytes(S, M, c["H"], c["W"]),), dtype=torch.uint8, device=cuda)
    runs = []
    for _ in range(2):                                                  # a stale workspace: all-zero keys would win everywhere
        out = projective.model_build(_dev(c["map_v"], cuda), _dev(c["map_n"], cuda), _dev(c["A"], cuda), _dev(c["live"], cuda),
                                     workspace=ws, **c["fov"])
        runs.append([t.cpu().numpy() for t in out])
        ws.zero_()
    mv, mn, src = runs[0]
    for s in range(S):
        want = model.model_build(c["map_v"][s], c["map_n"][s], c["A"][s], c["live"][s], c["im"])
        assert np.array_equal(src[s], want["src"]), (c["edge"], s)
        for got, exact in ((mv[s], want["v"]), (mn[s], want["n"])):
            ulp = np.spacing(np.abs(exact).astype(F)).astype(np.float64)
            assert (np.abs(got.astype(np.float64) - exact) <= ulp).all()
            if c["identity"]:
                assert _same(got, exact.astype(F))
        dead = c["live"][s] == 0
        assert (src[s, dead] == -1).all() and not mv[s, dead].any() and not mn[s, dead].any()
        for m in range(M):
            for name, t in c.get("plants", {}).get((s, m), {}).items():
                assert src[s, m].reshape(-1)[t[0]] == {"tie": t[1], "nearer": t[-1], "farther": t[2]}[name], name
    if "gone" in c:
        assert not np.isin(src, c["gone"]).any() and src.reshape(-1)[2 * c["W"]] == -1
    assert all(_same(a, b) for a, b in zip(*runs))


# ---- accumulate ----------------------------------------------------------------------------------------------------------------

ACC = C.accumulate_cases()


@pytest.mark.parametrize("c", ACC, ids=_ids(ACC))
def test_accumulate(cuda, c):
    S, HW = c["vmap"].shape[0], c["H"] * c["W"]
    runs = []
    for _ in range(2):
        out = projective.accumulate(_dev(c["vmap"], cuda), _dev(c["model_v"], cuda), _dev(c["model_n"], cuda),
                                    _dev(c["T"], cuda), sigma=c["sigma"], max_dist=c["max_dist"], with_pairs=True, **c["fov"])
        runs.append([t.cpu().numpy() for t in out])
    partial, slot, pixel = runs[0]
    G = registration.groups(HW)
    assert partial.shape == (S, G, 32) and G == (HW + 255) // 256
    assert np.isfinite(partial).all() and not partial[:, :, 30:].any()
    for s in range(S):
        want, mag, a = model.accumulate(c["vmap"][s], c["model_v"][s], c["model_n"][s], c["T"][s], c["im"], c["sigma"],
                                        c["max_dist"])
        assert np.array_equal(slot[s].reshape(-1), a["slot"]), (c["edge"], s)
        assert np.array_equal(pixel[s].reshape(-1), a["own_pixel"]), (c["edge"], s)
        row = partial[s].sum(axis=0)
        assert row[icp.PAIRS] == want[icp.PAIRS] and (np.abs(row - want) <= 1e-12 * mag).all(), (c["edge"], s)
        if want[icp.PAIRS] == 0:
            assert (_bits(partial[s]) == 0).all()                       # no pair at all: an all-zero row
    for (s, i), m in c["slot"].items():
        assert slot[s].reshape(-1)[i] == m
    for (s, i), p in c["pixel"].items():
        assert pixel[s].reshape(-1)[i] == p
    if "pairs" in c:
        assert partial.sum(axis=1)[:, icp.PAIRS].tolist() == list(c["pairs"])
    assert all(_same(a, b) for a, b in zip(*runs))


# ---- map push ------------------------------------------------------------------------------------------------------------------

PUSH = C.push_cases()


def _push(cuda, c, t):
    projective.map_push(_dev(c["T"], cuda), _dev(c["vmap"], cuda), _dev(c["nmap"], cuda), *[t[k] for k in
                                                                                           ("map_v", "map_n", "A", "live", "cursor")])


@pytest.mark.parametrize("c", PUSH, ids=_ids(PUSH))
def test_map_push(cuda, c):
    M = c["M"]
    keys = ("map_v", "map_n", "A", "live", "cursor")
    want = {k: c[k].copy() for k in keys}
    model.map_push(c["T"], c["vmap"], c["nmap"], **want)
    t = {k: _dev(c[k], cuda) for k in keys}
    _push(cuda, c, t)
    got = {k: t[k].cpu().numpy() for k in keys}
    assert _same(got["map_v"], want["map_v"]) and _same(got["map_n"], want["map_n"])        # the target new, the others as before
    assert np.array_equal(got["live"], want["live"]) and np.array_equal(got["cursor"], want["cursor"])
    assert np.abs(got["A"] - want["A"]).max() < 1e-12
    for s, m in enumerate(c["target"]):
        assert _same(got["map_v"][s, m], c["vmap"][s]) and _same(got["map_n"][s, m], c["nmap"][s])
        assert _same(got["A"][s, m], np.eye(4)) and got["live"][s, m] == 1 and got["cursor"][s] == (m + 1) % M
        others = np.arange(M) != m
        assert _same(got["map_v"][s, others], c["map_v"][s, others]) and _same(got["map_n"][s, others], c["map_n"][s, others])
        dead = others & (c["live"][s] == 0)
        assert _same(got["A"][s, dead], c["A"][s, dead])                # a dead slot's pose: untouched


def test_map_push_one_slot_three_times(cuda):
    c = C.push(1, 0)
    keys = ("map_v", "map_n", "A", "live", "cursor")
    t = {k: _dev(c[k], cuda) for k in keys}
    for turn in range(3):
        frame = dict(c, vmap=c["vmap"] + F(turn), nmap=c["nmap"] - F(turn))
        _push(cuda, frame, t)
        assert t["cursor"].tolist() == [0, 0, 0] and t["live"].tolist() == [[1]] * 3
        assert _same(t["map_v"].cpu().numpy()[:, 0], frame["vmap"]) and _same(t["map_n"].cpu().numpy()[:, 0], frame["nmap"])
        assert _same(t["A"].cpu().numpy(), np.tile(np.eye(4), (3, 1, 1, 1)))


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def test_refused_arguments_raise_before_any_launch(cuda):
    H, W, S, M = 2, 3, 2, 2
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device=cuda)
    pts, lengths = f(S, 4, 3), torch.full((S,), 4, dtype=torch.int32, device=cuda)
    vmap, images = f(S, H, W, 3), f(S, M, H, W, 3)
    T = torch.eye(4, dtype=torch.float64, device=cuda).expand(S, 4, 4).contiguous()
    A = torch.eye(4, dtype=torch.float64, device=cuda).expand(S, M, 4, 4).contiguous()
    live = torch.ones((S, M), dtype=torch.int32, device=cuda)
    calls, real = [], _lib.call
    _lib.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        with pytest.raises(ValueError, match="kernel_size=4"):
            projective.normal_map(vmap, kernel_size=4)
        with pytest.raises(ValueError, match="M=65"):
            projective.model_build(f(1, 65, H, W, 3), f(1, 65, H, W, 3), A[:1, :1].expand(1, 65, 4, 4).contiguous(),
                                   torch.ones((1, 65), dtype=torch.int32, device=cuda))
        with pytest.raises(ValueError, match="points"):
            projective.vertex_map(f(S, 4, 5), lengths=lengths, height=H, width=W)
        with pytest.raises(ValueError, match="sigma"):
            projective.accumulate(vmap, images, images, T, sigma=0.0)
        with pytest.raises(ValueError, match="max_dist"):
            projective.accumulate(vmap, images, images, T, max_dist=-0.5)
        with pytest.raises(ValueError, match="up_fov"):
            projective.vertex_map(pts, lengths=lengths, height=H, width=W, up_fov=0.0, down_fov=0.0)
        with pytest.raises(ValueError, match="vmap must be contiguous"):
            projective.accumulate(f(S, W, H, 3).transpose(1, 2), images, images, T)
        with pytest.raises(ValueError, match="lengths"):
            projective.vertex_map(pts, height=H, width=W)
        assert calls == []                                              # the Python layer refused all of these itself
    finally:
        _lib.call = real
    _lib.synchronize(cuda)
