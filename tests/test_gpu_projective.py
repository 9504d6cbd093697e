"""GPU checks of the projective registration against the fixtures recorded from the reference
(tests/golden/projective_cases.npz) and the fp64 model of tests/projective_model.py.

Pixels come from fp32 atan2 / asin, whose last bit a NumPy restatement cannot promise.  Inputs the tests build themselves
are therefore kept >= 1e-3 px (fp64) from every rounding boundary -- the fixtures' own condition -- by emptying the few
pixels that are not.  In the whole registration the poses are the device's own, so there the model takes the device's
pixel for a point inside that band (their number is asserted to stay below 1 %) and everything outside it must agree."""
import os

import numpy as np
import pytest
import torch

import icp_model as icp
import projective_model as model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "projective_cases.npz")
BAND = 1e-3


def load_cases():
    z = np.load(GOLDEN)
    out = []
    for i in range(int(z["cases"])):
        c = {k[len("c%d_" % i):]: z[k] for k in z.files if k.startswith("c%d_" % i)}
        H, W, up, down = c["image"]
        c["im"] = model.image(int(H), int(W), float(up), float(down))
        c["fov"] = dict(up_fov=float(up), down_fov=float(down))
        out.append(c)
    return out


CASES = load_cases()
IDS = ["%dx%d_fov%g" % (c["im"]["H"], c["im"]["W"], c["image"][2]) for c in CASES]
DEV = "cuda:0"


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else \
        torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def rigid(r, angle, shift):
    return icp.pose(icp.rot(r.normal(size=3), angle), r.normal(size=3) * shift)


# ---- 1. vertex map -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_vertex_map_against_the_fixtures(c):
    from pwclonet_pylidarslam_amd import projective
    im, pts, lengths = c["im"], c["points"], c["lengths"]
    S, R, _ = pts.shape
    kw = dict(height=im["H"], width=im["W"], **c["fov"])
    vmap, rows = projective.vertex_map(dev(pts), lengths=dev(lengths), **kw)
    assert vmap.cpu().numpy().tobytes() == c["ref_vmap"].tobytes()                   # bit-equal to the reference's
    want = np.stack([model.vertex_map(pts[s], im, lengths[s])[1] for s in range(S)])
    assert np.array_equal(rows.cpu().numpy(), want)                                  # ties: the lowest row; empty: -1
    assert (want[-1] == -1).all() and not vmap[-1].any()
    keep = (np.arange(R)[None, :] < lengths[:, None]).astype(np.int32)
    v2, r2 = projective.vertex_map(dev(pts), keep=dev(keep), **kw)
    assert torch.equal(v2, vmap) and torch.equal(r2, rows)                           # the keep-mask form
    four = np.concatenate([pts, np.ones((S, R, 1), dtype=np.float32)], axis=2)       # (S, R, 4) rows
    v3, r3 = projective.vertex_map(dev(four), lengths=dev(lengths), keep=dev(keep), **kw)
    assert torch.equal(v3, vmap) and torch.equal(r3, rows)
    v4, r4 = projective.vertex_map(dev(pts), lengths=dev(lengths), **kw)
    assert torch.equal(v4, vmap) and torch.equal(r4, rows)                           # two runs: the same bits


# ---- 2. normal map -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", CASES, ids=IDS)
@pytest.mark.parametrize("k", [3, 5])
def test_normal_map_against_the_model(c, k, capsys):
    """Direction error 1 - |n . n_model| <= 4 x the reference's fp32 error on the same input (recorded reference normals
    against the same fp64 model), the project's usual bound for an fp32 result against float64."""
    from pwclonet_pylidarslam_amd import projective
    im = c["im"]
    H, W = im["H"], im["W"]
    vmaps = c["ref_vmap"]                                                            # the device's own, bit for bit (above)
    lonely = np.zeros((1, H, W, 3), dtype=np.float32)                                # pairs of pixels with one neighbour,
    d = model.beams(im).reshape(H, W, 3)                                             # at a corner, an edge and inside
    for (y, x) in [(0, 0), (H - 1, W // 2), (H // 2, W // 3)]:
        lonely[0, y, x], lonely[0, y, min(x + 1, W - 1)] = d[y, x] * 4.0, d[y, min(x + 1, W - 1)] * 4.2
    batch = np.concatenate([vmaps, lonely])
    out = projective.normal_map(dev(batch), kernel_size=k).cpu().numpy()
    ref_err, err, lim = 0.0, 0.0, 0.0
    for i, v in enumerate(batch):
        n, det = model.normal_map(v, k)
        nz = (n != 0).any(axis=-1)
        assert np.array_equal(nz, (out[i] != 0).any(axis=-1))                        # border pixels included
        if i == len(batch) - 1:
            assert not nz.any()                                                      # one occupied neighbour: zero
        if nz.any():
            err = max(err, float((1.0 - np.abs((n[nz] * out[i][nz]).sum(axis=-1))).max()))
            assert np.abs(np.linalg.norm(out[i][nz].astype(np.float64), axis=-1) - 1.0).max() < 1e-6
            assert ((out[i][nz] * v[nz]).sum(axis=-1) > 0).all()                     # away from the sensor
        if i < len(vmaps) and nz.any():
            ref = c["ref_nmap%d" % k][i].astype(np.float64)
            ref_err = max(ref_err, float((1.0 - np.abs((n[nz] * ref[nz]).sum(axis=-1))).max()))
    with capsys.disabled():
        print("\n[projective] normal map %dx%d k=%d: device error %.3e, reference fp32 error %.3e, ratio %.3g"
              % (H, W, k, err, ref_err, err / ref_err))
    assert err <= 4.0 * ref_err


# ---- 3. model build ----------------------------------------------------------------------------------------------------------

def planted_map(c, seed, identity=False):
    """S = 2, M = 3 from the fixture's images: slot 1 dead, non-trivial A; pixels whose moved point lies inside the band
    are emptied first."""
    from pwclonet_pylidarslam_amd import projective
    r = np.random.default_rng([seed, c["im"]["H"], c["im"]["W"]])
    v = c["ref_vmap"]
    map_v = np.stack([v[[0, 1, 2]], v[[2, 0, 1]]]).copy()
    A = np.stack([np.stack([np.eye(4) if identity else rigid(r, 0.03, 0.15) for _ in range(3)]) for _ in range(2)])
    live = np.array([[1, 0, 1], [1, 0, 1]], dtype=np.int32)
    if identity:
        live[:] = 1
    for s in range(2):
        for m in range(3):
            inv = model.inverse(A[s, m])
            p = map_v[s, m].reshape(-1, 3)
            moved = (p.astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
            p[model.pixels(moved, c["im"])[4] < BAND] = 0.0
    map_n = projective.normal_map(dev(map_v.reshape(6, *v.shape[1:])), 5).cpu().numpy().reshape(map_v.shape)
    return map_v, map_n, A, live


@pytest.mark.parametrize("c", CASES[:2], ids=IDS[:2])
def test_model_build_against_the_model(c):
    from pwclonet_pylidarslam_amd import projective
    map_v, map_n, A, live = planted_map(c, 3)
    mv, mn, src = [t.cpu().numpy() for t in projective.model_build(dev(map_v), dev(map_n), dev(A), dev(live), **c["fov"])]
    for s in range(2):
        want = model.model_build(map_v[s], map_n[s], A[s], live[s], c["im"])
        assert np.array_equal(src[s], want["src"])                                   # pixels and winners
        assert (src[s, 1] == -1).all() and not mv[s, 1].any() and not mn[s, 1].any()     # the dead slot: an empty image
        assert (src[s, 0] >= 0).sum() > src[s, 0].size // 4
        for got, exact in ((mv[s], want["v"]), (mn[s], want["n"])):
            ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
            assert (np.abs(got.astype(np.float64) - exact) <= ulp).all()             # one rounding of the fp64 product
    map_v, map_n, A, live = planted_map(c, 3, identity=True)
    mv, mn, src = [t.cpu().numpy() for t in projective.model_build(dev(map_v), dev(map_n), dev(A), dev(live), **c["fov"])]
    assert mv.tobytes() == map_v.tobytes() and mn.tobytes() == map_n.tobytes()       # A = I: bit-equal
    HW = c["im"]["H"] * c["im"]["W"]
    occupied = (map_v != 0).any(axis=-1).reshape(2, 3, HW)
    assert np.array_equal(src.reshape(2, 3, HW), np.where(occupied, np.arange(HW), -1))


# ---- 4. accumulate -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", CASES[:2], ids=IDS[:2])
def test_accumulate_against_the_model(c):
    """n = H * W (5 x 60 leaves a partial workgroup), three streams; the last one's model is empty: a zero row."""
    from pwclonet_pylidarslam_amd import projective, registration
    im = c["im"]
    H, W = im["H"], im["W"]
    map_v2, map_n2, A2, live2 = planted_map(c, 5)
    map_v, map_n = np.concatenate([map_v2, map_v2[:1]]), np.concatenate([map_n2, map_n2[:1]])
    A, live = np.concatenate([A2, A2[:1]]), np.concatenate([live2, np.zeros((1, 3), dtype=np.int32)])
    model_v, model_n, _ = [t.cpu().numpy() for t in projective.model_build(dev(map_v), dev(map_n), dev(A), dev(live),
                                                                         **c["fov"])]
    r = np.random.default_rng([7, H, W])
    T = np.stack([rigid(r, 0.02, 0.1) for _ in range(3)])
    vmap = c["ref_vmap"][[1, 2, 0]].copy()
    for s in range(3):                                                               # moved points out of the band
        a = model.associate(vmap[s], model_v[s], model_n[s], T[s], im, 1.0)
        vmap[s].reshape(-1, 3)[a["margin"] < BAND] = 0.0
    partial, slot, pixel = projective.accumulate(dev(vmap), dev(model_v), dev(model_n), dev(T), sigma=0.05, max_dist=1.0,
                                                 with_pairs=True, **c["fov"])
    G = registration.groups(H * W)
    assert partial.shape == (3, G, 32) and (G > 1 or H * W <= 256)
    rows = partial.cpu().numpy().sum(axis=1)
    status = torch.zeros((3,), dtype=torch.int32, device=DEV)
    Td = dev(T.copy())
    out = registration.solve(partial, Td, status, it=0, min_pairs=16)                # the existing solver takes the rows
    for s in range(3):
        want, mag, a = model.accumulate(vmap[s], model_v[s], model_n[s], T[s], im, 0.05, 1.0)
        assert np.array_equal(slot[s].cpu().numpy().reshape(-1), a["slot"])
        assert np.array_equal(pixel[s].cpu().numpy().reshape(-1), a["own_pixel"])
        assert (np.abs(rows[s] - want) <= 1e-12 * mag).all()
        assert np.array_equal(out["sum"][s].cpu().numpy(), rows[s]) or np.allclose(out["sum"][s].cpu().numpy(), rows[s],
                                                                                   rtol=1e-15, atol=0)
        if s == 2:
            assert not partial[s].cpu().numpy().any() and (a["slot"] == -1).all()    # no pairs: a zero row
            continue
        assert want[icp.PAIRS] > 100 and (np.abs(want[icp.G0:icp.G0 + 6]) > 0).all()
        ms = icp.solve(want, T[s], 0, 0, 1e-6, 1e-4, 16)
        assert np.abs(out["delta"][s].cpu().numpy() - ms["delta"]).max() < 1e-10
        assert np.abs(Td[s].cpu().numpy() - ms["T"]).max() < 1e-10
    assert status.cpu().numpy().tolist()[2] == icp.FEW_PAIRS


# ---- 5. whole registration ---------------------------------------------------------------------------------------------------

ROOM_IM = model.image(16, 64, 3.0, -24.8)
ROOM_FOV = dict(up_fov=3.0, down_fov=-24.8)
FRAMES, STREAMS, SLOTS, ITERS = 4, 2, 3, 10


@pytest.fixture(scope="module")
def room():
    """Two streams' scans of the box room (16 x 64 beams, 0.01 m range noise), four frames each: one to fill the map and
    three to register; guesses off by 2 degrees and 0.3 m.  The fp64 model's own run on these frames, on the CPU first."""
    scans = [model.room_scans(31 + s, FRAMES, ROOM_IM) for s in range(STREAMS)]
    clouds = np.stack([sc[0] for sc in scans], axis=1)                               # (frames, S, HW, 3)
    gt = np.stack([sc[1] for sc in scans], axis=1)
    guess = np.stack([[icp.perturbed(gt[k, s]) for s in range(STREAMS)] for k in range(FRAMES)])
    maps = [model.Map(SLOTS, 16, 64) for _ in range(STREAMS)]
    errs, guess_errs = [], []
    for k in range(FRAMES):
        for s in range(STREAMS):
            vmap, _ = model.vertex_map(clouds[k, s], ROOM_IM, clouds.shape[2])
            nmap = model.normal_map(vmap, 5)[0].astype(np.float32)
            T, status, _ = model.register(maps[s], vmap, nmap, guess[k, s], ROOM_IM, iters=ITERS, min_pairs=64)
            if k > 0:
                errs.append(icp.pose_error(T, gt[k, s]))
                guess_errs.append(icp.pose_error(guess[k, s], gt[k, s]))
    return dict(clouds=clouds, gt=gt, guess=guess, model_err=np.array(errs).reshape(FRAMES - 1, STREAMS),
                guess_err=np.array(guess_errs).reshape(FRAMES - 1, STREAMS))


def run_refiner(room, graph, trace=False):
    from pwclonet_pylidarslam_amd import projective
    n = room["clouds"].shape[2]
    ref = projective.ProjectiveIcpRefiner(STREAMS, n, height=16, width=64, map_size=SLOTS, iters=ITERS, graph=graph,
                                          **ROOM_FOV)
    lengths = torch.full((STREAMS,), n, dtype=torch.int32, device=DEV)
    out = []
    for k in range(FRAMES):
        res = ref.register(dev(room["clouds"][k]), lengths, dev(room["guess"][k]), trace=trace)
        T, tr = res if trace else (res, None)
        state = {key: v.cpu().numpy().copy() for key, v in ref.map_state().items()}
        out.append(dict(T=T.cpu().numpy().copy(), trace=tr, status=ref.status().cpu().numpy().copy(), **state))
    return ref, out


def test_whole_registration_teacher_forced(room, capsys):
    """Every iteration is checked from the device's own pose before it; the model is fed the device's model images (checked
    against its own outside the band) so that one frame's in-band pixel cannot hide the next comparison."""
    assert (room["model_err"] < room["guess_err"]).all()                             # the condition: the model improves
    _, eager = run_refiner(room, graph=False, trace=True)
    maps = [model.Map(SLOTS, 16, 64) for _ in range(STREAMS)]
    in_band = total = 0
    for k in range(FRAMES):
        tr = eager[k]["trace"]
        for s in range(STREAMS):
            vmap, rows = model.vertex_map(room["clouds"][k, s], ROOM_IM, room["clouds"].shape[2])
            assert tr["vmap"][s].cpu().numpy().tobytes() == vmap.tobytes()
            assert np.array_equal(tr["rows"][s].cpu().numpy(), rows)
            nmap = tr["nmap"][s].cpu().numpy()
            n64 = model.normal_map(vmap, 5)[0]
            assert np.array_equal((nmap != 0).any(axis=-1), (n64 != 0).any(axis=-1))
            built = model.model_build(maps[s].v, maps[s].n, maps[s].A, maps[s].live, ROOM_IM)
            mv, mn = tr["model_v"][s].cpu().numpy(), tr["model_n"][s].cpu().numpy()
            src = tr["model_src"][s].cpu().numpy()
            differ = (src != built["src"]).reshape(SLOTS, -1)
            for m in range(SLOTS):                                                   # a differing pixel has a cause inside
                for p in np.flatnonzero(differ[m]):                                  # the band: a source that lands on it
                    cand = [i for i in (src[m].reshape(-1)[p], built["src"][m].reshape(-1)[p]) if i >= 0]
                    assert any(built["margin"][m][i] < BAND for i in cand)
            total += src.size
            in_band += int(differ.sum())
            status = 0
            for it, step in enumerate(tr["steps"]):
                Tb = step["T_before"][s].cpu().numpy()
                dev_pix = step["pixel"][s].cpu().numpy().reshape(-1).astype(np.int64)
                a = model.associate(vmap, mv, mn, Tb, ROOM_IM, 1.0)
                near = a["margin"] < BAND
                assert np.array_equal(dev_pix[~near], a["own_pixel"][~near])
                pix = np.where(near, dev_pix, a["own_pixel"])
                total += pix.size
                in_band += int((dev_pix != a["own_pixel"]).sum())
                row, mag, a = model.accumulate(vmap, mv, mn, Tb, ROOM_IM, 0.5, 1.0, pixel=pix)
                assert np.array_equal(step["slot"][s].cpu().numpy().reshape(-1), a["slot"])
                assert (np.abs(step["sum"][s].cpu().numpy() - row) <= 1e-12 * mag + 1e-300).all()
                ms = icp.solve(step["sum"][s].cpu().numpy(), Tb, status, it, 1e-6, 1e-4, 64)
                status = ms["status"]
                assert np.abs(step["T"][s].cpu().numpy() - ms["T"]).max() < 1e-10
                assert int(step["status"][s]) == status
            maps[s].push(vmap, nmap, eager[k]["T"][s])
            assert np.abs(eager[k]["A"][s] - maps[s].A).max() < 1e-12               # after every push
            assert np.array_equal(eager[k]["live"][s], maps[s].live) and eager[k]["cursor"][s] == maps[s].cursor
            maps[s].A = eager[k]["A"][s].copy()
    assert in_band <= 0.01 * total
    dev_err = np.array([[icp.pose_error(eager[k]["T"][s], room["gt"][k, s]) for s in range(STREAMS)]
                        for k in range(1, FRAMES)])
    with capsys.disabled():
        print("\n[projective] room: device error / model error max %.3f; error / guess error max %.3f (model %.3f); "
              "in-band decisions %d of %d" % ((dev_err / room["model_err"]).max(), (dev_err / room["guess_err"]).max(),
                                             (room["model_err"] / room["guess_err"]).max(), in_band, total))
    assert (dev_err <= 1.5 * room["model_err"]).all()


def test_whole_registration_eager_graph_and_rerun_bit_equal(room):
    ref, graph = run_refiner(room, graph=True)
    _, eager = run_refiner(room, graph=False)
    _, again = run_refiner(room, graph=True)
    assert ref.captures == 1 and ref.calls == FRAMES
    for k in range(FRAMES):
        for key in ("T", "A", "live", "cursor", "status"):
            assert graph[k][key].tobytes() == eager[k][key].tobytes() == again[k][key].tobytes(), (k, key)


# ---- 6. first frame and reset ------------------------------------------------------------------------------------------------

def test_first_frame_and_reset(room):
    from pwclonet_pylidarslam_amd import projective
    n = room["clouds"].shape[2]
    ref = projective.ProjectiveIcpRefiner(STREAMS, n, height=16, width=64, map_size=SLOTS, iters=3, graph=False, **ROOM_FOV)
    lengths = [n] * STREAMS
    assert ref.status() is None and ref.map_state() is None
    for round_ in range(2):
        init = dev(room["guess"][1])
        T = ref.register(dev(room["clouds"][0]), lengths, init)
        assert T.cpu().numpy().tobytes() == room["guess"][1].tobytes()               # init, bit for bit
        assert (ref.status().cpu().numpy() == icp.FEW_PAIRS).all()
        state = ref.map_state()
        assert state["live"].cpu().numpy().tolist() == [[1, 0, 0]] * STREAMS         # slot 0 is filled
        assert state["cursor"].cpu().numpy().tolist() == [1] * STREAMS
        assert ref.diagnostics()["pairs"].cpu().numpy().tolist() == [0] * STREAMS
        T = ref.register(dev(room["clouds"][1]), lengths, dev(room["guess"][1]))
        assert (ref.diagnostics()["pairs"].cpu().numpy() > 64).all()
        assert ref.map_state()["live"].cpu().numpy().tolist() == [[1, 1, 0]] * STREAMS
        ref.reset()
    with pytest.raises(ValueError, match="lock step only"):
        projective.ProjectiveIcpRefiner(STREAMS, n, per_stream=True)
    with pytest.raises(ValueError, match="trace"):
        projective.ProjectiveIcpRefiner(STREAMS, n, height=16, width=64).register(dev(room["clouds"][0]), lengths,
                                                                                  dev(room["guess"][0]), trace=True)
