"""GPU tests of the loop detector's kernels: the descriptor and the search against the same-order fp32
model of tests/loop_closure_model.py, bit for bit, and the database's bookkeeping.  The decisions compared here carry the fp64
margins that tests/test_loop_closure_cpu.py asserts."""
import numpy as np
import pytest
import torch

import loop_closure_cases as C
import loop_closure_model as M
from pwclonet_pylidarslam_amd import loop_closure as L

pytestmark = pytest.mark.gpu
F = np.float32


def _mask_int(v):
    return int(v) & ((1 << 64) - 1)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)


def _cloud(seed, n, rings, sectors, z_offset=C.Z_OFFSET):
    """Random rows with the edge rows mixed in (as many as fit), shuffled: the maximum does not depend on the order."""
    edge = C.edge_rows(rings, sectors, z_offset=z_offset)
    rng = np.random.default_rng(seed)
    c = C.random_cloud(seed, n)
    k = min(len(edge), n - n // 4)
    at = rng.permutation(n)[:k]
    c[at] = edge[rng.permutation(len(edge))[:k]] if k < len(edge) else edge
    return c


@pytest.mark.parametrize("rings,sectors", C.SHAPES)
@pytest.mark.parametrize("n", [64, 65, 1000, 8192])
@pytest.mark.parametrize("S", [1, 3])
def test_descriptor_bits(cuda, S, n, rings, sectors):
    clouds = np.stack([_cloud(7 * s + n, n, rings, sectors) for s in range(S)])
    D, Dn, mask = L.scan_context(torch.from_numpy(clouds).to(cuda), rings, sectors)
    for s in range(S):
        d, dn, m = M.descriptor(clouds[s], rings, sectors)
        assert np.array_equal(_bits(D[s].cpu().numpy()), _bits(d)), (s, "D")
        assert np.array_equal(_bits(Dn[s].cpu().numpy()), _bits(dn)), (s, "Dn")
        assert _mask_int(mask[s]) == m
    assert (D.cpu().numpy() > 0).any()


def test_descriptor_edges_lengths_and_camera_frame(cuda):
    rings, sectors = 20, 60
    for z_offset in (C.Z_OFFSET, 0.0):                  # 0: the smallest positive float is a height
        rows = C.edge_rows(rings, sectors, z_offset=z_offset)
        d, dn, m = M.descriptor(rows, rings, sectors, z_offset=z_offset)
        D, Dn, mask = L.scan_context(torch.from_numpy(rows[None]).to(cuda), rings, sectors, z_offset=z_offset)
        assert np.array_equal(_bits(D[0].cpu().numpy()), _bits(d)) and np.array_equal(_bits(Dn[0].cpu().numpy()), _bits(dn))
        assert _mask_int(mask[0]) == m
        cam = C.to_camera(rows).astype(F)
        Dc, Dnc, maskc = L.scan_context(torch.from_numpy(cam[None]).to(cuda), rings, sectors, z_offset=z_offset, up="-y")
        assert torch.equal(Dc, D) and torch.equal(Dnc, Dn) and torch.equal(maskc, mask)
    # a length shorter than n: the rows behind it would raise maxima and fill cells
    clouds = np.stack([_cloud(s, 300, rings, sectors) for s in range(3)])
    clouds[:, 200:, 2] += 3.0
    lengths = np.array([200, 0, 1000], dtype=np.int32)
    D, Dn, mask = L.scan_context(torch.from_numpy(clouds).to(cuda), rings, sectors, lengths=torch.from_numpy(lengths).to(cuda))
    for s in range(3):
        d, dn, m = M.descriptor(clouds[s], rings, sectors, length=lengths[s])
        assert np.array_equal(_bits(D[s].cpu().numpy()), _bits(d)) and _mask_int(mask[s]) == m
        assert not np.array_equal(d, M.descriptor(clouds[s], rings, sectors)[0]) or s == 2
    assert _mask_int(mask[1]) == 0 and not D[1].any()


def _detector(cuda, S, n, rings, sectors, **kw):
    det = L.ScanContextLoopDetector(S, n, rings, sectors, device=cuda, **dict(dict(verify=None, min_id_distance=C.MIN_ID), **kw))
    det._alloc()
    return det


def _load(det, s, Dn, masks, frame_ids):
    """Places straight into stream s of the database, as insert lays them out."""
    b, c = det.bufs, len(masks)
    if c:
        b["db_desc"][s, :c].copy_(torch.from_numpy(np.ascontiguousarray(np.transpose(Dn, (0, 2, 1)))))
        signed = np.array([m - (1 << 64) if m >> 63 else m for m in masks], dtype=np.int64)
        b["db_mask"][s, :c].copy_(torch.from_numpy(signed))
        b["db_frame"][s, :c].copy_(torch.from_numpy(np.asarray(frame_ids, dtype=np.int32)))
    b["count"][s:s + 1].fill_(c)


def _query(det, clouds, frame_ids, trajectory=None, active=None):
    b = det.bufs
    b["cloud"].copy_(torch.from_numpy(np.ascontiguousarray(clouds, dtype=F)))
    b["frame_id"].copy_(torch.tensor(frame_ids, dtype=torch.int32))
    b["lengths"].fill_(det.num_points)
    b["active"].copy_(torch.tensor([1] * det.streams if active is None else active, dtype=torch.int32))
    det.search(trajectory)


def _expect(det, s, out, count):
    b = det.bufs
    scores, shifts = b["scores"][s, :count].cpu().numpy(), b["shifts"][s, :count].cpu().numpy()
    assert np.array_equal(_bits(scores), _bits(out["scores"])), (s, "scores")
    assert np.array_equal(shifts, out["shifts"]), (s, "shifts")
    assert np.isinf(b["scores"][s, count:].cpu().numpy()).all()
    m = det.match()
    got = tuple(int(m[k][s]) for k in ("found", "entry", "frame_i", "shift"))
    assert got == (out["found"], out["entry"], out["frame_i"], out["shift"]), (s, got, out)
    assert _bits(m["score"][s].cpu().numpy()) == _bits(F(out["score"]))
    want = M.start_pose(out["shift"], det.sectors, det.up) if out["found"] else np.eye(4)
    assert np.abs(m["T0"][s].cpu().numpy() - want).max() <= 1e-15


@pytest.mark.parametrize("count", C.SEARCH_COUNTS)
def test_search_bits(cuda, count):
    """Databases of 1, 63, 64, 65 and 257 places; stream 1 holds the same places in reverse order, stream 2 none."""
    rings, sectors = C.SEARCH_SHAPE
    c = C.search_case(count)
    det = _detector(cuda, 3, C.SEARCH_N, rings, sectors, max_keyframes=260)
    _load(det, 0, c["Dn"], c["masks"], c["frame_ids"])
    _load(det, 1, c["Dn"][::-1], c["masks"][::-1], c["frame_ids"])
    _query(det, np.stack([c["query"]] * 3), [c["f"]] * 3)
    _, Qn, qmask = M.descriptor(c["query"], rings, sectors)
    assert np.array_equal(_bits(det.bufs["Dn"][0].cpu().numpy()), _bits(Qn))
    out = M.search(Qn, qmask, c["Dn"], c["masks"], c["frame_ids"], c["f"], C.MIN_ID, det.threshold)
    assert (out["entry"], out["shift"], out["found"]) == (c["want"], c["shift"], 1)
    _expect(det, 0, out, count)
    _expect(det, 1, M.search(Qn, qmask, c["Dn"][::-1], c["masks"][::-1], c["frame_ids"], c["f"], C.MIN_ID, det.threshold), count)
    _expect(det, 2, M.search(Qn, qmask, [], [], [], c["f"], C.MIN_ID, det.threshold), 0)          # an empty database
    assert det.bufs["slot"].tolist() == [count, count, 0]


def test_search_rules(cuda):
    rings, sectors, n = 4, 8, 64
    Dn, masks, clouds = C.places(7, 3, rings, sectors, n)
    En, em = np.stack([Dn[0], Dn[1], Dn[1]]), [masks[0], masks[1], masks[1]]
    ring_only = np.zeros((n, 3), dtype=F)
    ang = (np.arange(n) % sectors + 0.5) * 2 * np.pi / sectors
    ring_only[:, 0], ring_only[:, 1], ring_only[:, 2] = 30.0 * np.cos(ang), 30.0 * np.sin(ang), 0.5
    sym = M.descriptor(ring_only, rings, sectors)
    empty = np.zeros((n, 3), dtype=F)
    pos = np.zeros((31, 3))
    pos[30] = (3.0, 4.0, 0.0)
    traj = np.tile(np.eye(4), (31, 5, 1, 1))
    traj[:, :, :3, 3] = pos[:, None, :]
    traj = torch.from_numpy(traj).to(cuda)

    def run(queries, ids, dbs, threshold=0.2, max_distance=None, trajectory=None, min_id=5):
        S = len(queries)
        det = _detector(cuda, S, n, rings, sectors, max_keyframes=8, threshold=threshold, max_distance=max_distance,
                        min_id_distance=min_id)
        for s, (E, msk, fid) in enumerate(dbs):
            _load(det, s, E, msk, fid)
        _query(det, np.stack(queries), [30] * S, trajectory)
        for s, (E, msk, fid) in enumerate(dbs):
            q = M.descriptor(queries[s], rings, sectors)
            p = None if trajectory is None else pos
            _expect(det, s, M.search(q[1], q[2], E, msk, fid, 30, min_id, threshold, p, max_distance), len(msk))
        return det.match()

    same = (En, em, [0, 1, 2])
    m = run([clouds[1], ring_only, empty, clouds[1], clouds[1]],
            None, [same, (sym[1][None], [sym[2]], [0]), same, (En, em, [25, 26, 27]), (En, em, [26, 27, 28])])
    assert m["entry"].tolist() == [1, 0, -1, 0, -1] and m["found"].tolist()[:3] == [1, 1, 0] and int(m["found"][4]) == 0
    assert int(m["shift"][1]) == 0 and np.isinf(float(m["score"][2]))
    m = run([clouds[1]] * 5, None, [same] * 5, max_distance=5.0, trajectory=traj[:, :5].contiguous())
    assert m["entry"].tolist() == [-1] * 5                                # exactly max_distance away: not eligible
    m = run([clouds[1]] * 5, None, [same] * 5, max_distance=float(np.nextafter(5.0, 6.0)), trajectory=traj[:, :5].contiguous())
    assert m["entry"].tolist() == [1] * 5
    score = M.search(Dn[0], masks[0], [Dn[1]], [masks[1]], [0], 30, 5, 0.2)["score"]
    one = (Dn[1][None], [masks[1]], [0])
    assert run([clouds[0]], None, [one], threshold=float(score))["found"].tolist() == [0]     # score == threshold: no match
    assert run([clouds[0]], None, [one], threshold=float(np.nextafter(score, F(2))))["found"].tolist() == [1]


def test_insert_stride_overflow_restart_and_idle(cuda):
    rings, sectors, n, S = 4, 8, 64, 3
    det = L.ScanContextLoopDetector(S, n, rings, sectors, max_keyframes=3, stride=2, min_id_distance=2, verify=None,
                                    device=cuda)
    clouds = [np.stack([C.pad(C.cell_centres(10 * f + s, rings, sectors), n) for s in range(S)]) for f in range(9)]
    state = lambda: {k: det.bufs[k].clone() for k in ("db_desc", "db_mask", "db_frame", "count", "nlog", "log_i", "log_T")}
    eager = []
    for f in range(5):                                   # frames 0, 2, 4 are stored (stride 2): counts 1, 1, 2, 2, 3
        det.process(torch.from_numpy(clouds[f]).to(cuda), [f] * S)
        eager.append(state())
        assert det.counts().tolist() == [f // 2 + 1] * S and not det.overflowed()
    assert det.captures == 1
    db = det.database(1)
    assert db["frame_id"].tolist() == [0, 2, 4]
    for e, f in enumerate((0, 2, 4)):
        _, dn, m = M.descriptor(clouds[f][1], rings, sectors)
        assert np.array_equal(_bits(db["Dn"][e].cpu().numpy()), _bits(dn)) and _mask_int(db["mask"][e]) == m
    # eager equals replay: a detector that never captures holds the same words after every call
    plain = L.ScanContextLoopDetector(S, n, rings, sectors, max_keyframes=3, stride=2, min_id_distance=2, verify=None,
                                      device=cuda, graph=False)
    for f in range(5):
        plain.process(torch.from_numpy(clouds[f]).to(cuda), [f] * S)
        for k, v in eager[f].items():
            assert torch.equal(plain.bufs[k], v), (f, k)
    assert plain.captures == 0
    # stream 1 idles with rows that would match; stream 0 restarts; stream 2 overflows (frame 6, a full database)
    before = state()
    det.process(torch.from_numpy(clouds[0]).to(cuda), [6] * S, active=[1, 0, 1], restart=[1, 0, 0])
    after = state()
    for k in before:
        assert torch.equal(after[k][1], before[k][1]), k                 # the idle stream keeps every word
        if k.startswith("db_") or k == "count":
            assert torch.equal(after[k][2], before[k][2]), k             # a full database: nothing written
    assert det.overflowed() and det.counts().tolist() == [1, 3, 3]
    assert det.database(0)["frame_id"].tolist() == [6]
    m = det.match()
    assert m["found"].tolist() == [0, 0, 1] and int(m["frame_i"][2]) == 0 and int(m["entry"][0]) == -1
    # verify=None: every match is logged with T0
    recs = det.loops()
    assert [(r.stream, r.i, r.j) for r in recs] == [(2, 0, 6)]
    assert [(r.stream, r.i, r.j, r.shift) for r in det.poll()] == [(2, 0, 6, recs[0].shift)] and det.poll() == []
    assert np.abs(recs[0].T - M.start_pose(recs[0].shift, sectors)).max() <= 1e-15 and recs[0].score < 1e-6
    det.reset([2])
    assert det.counts().tolist() == [1, 3, 0] and det.loops() == [] and det.poll() == []
