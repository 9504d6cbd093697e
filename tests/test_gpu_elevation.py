"""GPU tests of the translation search's kernels: the images, their cell counts and lists, every entry
of A, the record and T1 against tests/elevation_model.py, bit for bit; the inputs are the edge rows and the rule table that
tests/test_elevation_cpu.py checks on the model."""
import numpy as np
import pytest
import torch

import elevation_cases as EC
import elevation_model as EM
import loop_closure_cases as C
import loop_closure_model as LM
from pwclonet_pylidarslam_amd import loop_closure as L

pytestmark = pytest.mark.gpu
F = np.float32


def _run(cuda, p, stored, query, shifts, found, lengths=None, up="z", z_offset=EC.Z_OFFSET):
    """The three launches on buffers filled as select and fetch leave them -> (detector, T0 (S, 4, 4))."""
    S, n = len(query), query[0].shape[0]
    det = L.ScanContextLoopDetector(S, n, sectors=EC.SECTORS, z_offset=z_offset, up=up, max_keyframes=1, device=cuda,
                                    translation=p)
    det._alloc()
    b = det.bufs
    T0 = np.stack([LM.start_pose(shifts[s], EC.SECTORS, up) if found[s] else np.eye(4) for s in range(S)])
    b["staging"].copy_(torch.from_numpy(np.stack(stored).astype(F)))
    b["cloud"].copy_(torch.from_numpy(np.stack(query).astype(F)))
    b["lengths"].copy_(torch.tensor([n] * S if lengths is None else lengths, dtype=torch.int32))
    b["found"].copy_(torch.tensor(found, dtype=torch.int32))
    b["match"][:, 0].copy_(b["found"])
    b["match"][:, 3].copy_(torch.tensor(shifts, dtype=torch.int32))
    b["T0"].copy_(torch.from_numpy(T0))
    b["ei_record"].fill_(-7)                             # every word must be written, for the streams without a match too
    b["T1"].fill_(float("nan"))
    det.translate()
    return det, T0


def _expect(det, s, out):
    b, t = det.bufs, det.translation
    G = t["cells"]
    img, occ = b["ei_img"][s].cpu().numpy(), b["ei_occ"][s].cpu().numpy()
    assert np.array_equal(img[0], out["E"]), (s, "E")
    assert np.array_equal(img[1:], out["Q"]), (s, "Q")
    assert occ[0] == out["occ_e"] and np.array_equal(occ[1:], out["occ_q"]), (s, "occ")
    lists = b["ei_list"][s].cpu().numpy()
    for k in range(len(out["Q"])):                       # the list: every non-empty cell once, in any order
        w = np.sort(lists[k, :occ[1 + k]])
        i, j = np.nonzero(out["Q"][k])
        want = np.sort(i | (j << 8) | (out["Q"][k][i, j].astype(np.int64) << 16))
        assert np.array_equal(w, want), (s, k, "list")
    assert np.array_equal(b["ei_A"][s].cpu().numpy(), out["A"]), (s, "A")
    rec = out["record"]
    assert b["ei_record"][s].tolist() == [rec[k] for k in EM.RECORD] + [0], (s, b["ei_record"][s].tolist(), rec)
    assert b["T1"][s].cpu().numpy().tobytes() == np.ascontiguousarray(out["T1"]).tobytes(), (s, "T1")
    seed = det.seed()
    assert int(seed["found"][s]) == rec["found"] and int(seed["a"][s]) == rec["a"] and torch.equal(seed["T1"], b["T1"])


def _cloud(seed, n, p, extent=1.3):
    """Random rows over and a little beyond the grid, the edge rows mixed in (as many as fit), shuffled."""
    rng = np.random.default_rng(seed)
    half = extent * p["cells"] * p["cell_size"] / 2
    c = np.stack([rng.uniform(-half, half, n), rng.uniform(-half, half, n), rng.uniform(-3.0, 6.0, n)], axis=1).astype(F)
    edge = EC.edge_rows(p)
    k = min(len(edge), n // 2)
    c[rng.permutation(n)[:k]] = edge[rng.permutation(len(edge))[:k]]
    return c


@pytest.mark.parametrize("up", ["z", "-y"])
@pytest.mark.parametrize("n", [64, 65, 257])
def test_bits_with_short_lengths_and_a_stream_without_a_match(cuda, n, up):
    """S = 3 with found = (1, 0, 1): stream 1 keeps T0 to the bit and gets a record of zeros; the rows past a length would
    raise maxima and fill cells."""
    p = dict(EC.SMALL)
    stored = [_cloud(10 * n + s, n, p) for s in range(3)]
    query = [_cloud(10 * n + 5 + s, n, p) for s in range(3)]
    for q in query:
        q[n // 2:, 2] += 3.0
    lengths, shifts, found = [n // 2, n, n - 1], [7, 31, 59], [1, 0, 1]
    cam = (lambda c: C.to_camera(c).astype(F)) if up == "-y" else (lambda c: c)
    det, T0 = _run(cuda, p, [cam(c) for c in stored], [cam(c) for c in query], shifts, found, lengths, up)
    for s in (0, 2):
        out = EM.search(cam(stored[s]), cam(query[s]), shifts[s], EC.SECTORS, p, up=up, length=lengths[s])
        assert out["record"]["A"] > 0 and out["occ_e"] > 8
        _expect(det, s, out)
        whole = EM.search(cam(stored[s]), cam(query[s]), shifts[s], EC.SECTORS, p, up=up)
        assert s == 2 or not np.array_equal(whole["Q"], out["Q"])               # the length n // 2 decided something
    assert det.bufs["ei_record"][1].tolist() == [0] * 8
    assert det.bufs["T1"][1].cpu().numpy().tobytes() == T0[1].tobytes()


@pytest.mark.parametrize("cells,window,yaw_half", [(8, 0, 1), (8, 16, 1), (128, 16, 4), (16, 3, 0), (16, 3, 8), (10, 5, 2)])
def test_bits_at_every_shape(cuda, cells, window, yaw_half):
    """The smallest grid without a window and with a window larger than itself, the largest grid and window (an LDS image of
    64 KiB and a padded one of 25 KiB), one yaw candidate and seventeen, and a grid whose cell count is no multiple of the
    workgroup."""
    p = dict(EM.DEFAULTS, cells=cells, window=window, yaw_half=yaw_half, cell_size=0.5 if cells == 128 else 1.0)
    n = 300
    lat = EC.lattice(cells, p, margin=1 if cells <= 10 else 3)
    moved = EC.seen_from(lat, 11, yaw_half, 1 if window else 0, -1 if window else 0, p)
    stored = [_cloud(cells + window, n, p), C.pad(lat, n)]
    query = [_cloud(cells + window + 1, n, p), C.pad(moved, n)]
    det, _ = _run(cuda, p, stored, query, [44, 11], [1, 1])
    for s in range(2):
        out = EM.search(stored[s], query[s], [44, 11][s], EC.SECTORS, p)
        assert out["A"].shape == (2 * yaw_half + 1, 2 * window + 1, 2 * window + 1) and out["A"].any()
        _expect(det, s, out)
    rec = det.seed()
    assert int(rec["found"][1]) == 1 and (int(rec["a"][1]), int(rec["b"][1])) == ((1, -1) if window else (0, 0))


@pytest.mark.parametrize("up", ["z", "-y"])
def test_bits_on_the_rule_table(cuda, up):
    """The edge rows and the tie, empty and acceptance cases, as tests/test_elevation_cpu.py decides them on the model."""
    cam = (lambda c: C.to_camera(c).astype(F)) if up == "-y" else (lambda c: c)
    for case in EC.rule_cases():
        n = 128
        m = len(case["query"]) if case["length"] is None else case["length"]
        query = C.pad(case["query"][:m], n)              # repeats of the rows that count change no maximum
        stored = C.pad(case["stored"], n)
        det, _ = _run(cuda, case["p"], [cam(stored)], [cam(query)], [case["shift"]], [1], up=up)
        out = EM.search(cam(case["stored"]), cam(case["query"]), case["shift"], EC.SECTORS, case["p"], up=up, length=case["length"])
        _expect(det, 0, out)
