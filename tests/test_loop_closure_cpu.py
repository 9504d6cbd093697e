"""The loop detector without a GPU: the fp32 model against a plain fp64 restatement, the yaw sign, the
``up="-y"`` permutation, every host refusal, the ABI, the reference-interface class on a stub, and the fp64 margins of every
decision the GPU tests compare."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_closure_cases as C          # noqa: E402
import loop_closure_model as M          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["scan_context_build_kernel_wrapper", "loop_score_kernel_wrapper", "loop_select_kernel_wrapper",
       "loop_fetch_kernel_wrapper", "loop_accept_kernel_wrapper", "loop_insert_kernel_wrapper"]


@pytest.mark.parametrize("rings,sectors", C.SHAPES)
def test_model_agrees_with_the_fp64_restatement(rings, sectors):
    """Points at cell centres are far from every bin edge, so both binnings agree and only rounding separates the two."""
    clouds = [C.cell_centres(s, rings, sectors).astype(np.float32) for s in (1, 2, 3)]
    d32 = [M.descriptor(c, rings, sectors) for c in clouds]
    d64 = [M.descriptor64(c, rings, sectors) for c in clouds]
    for a, b in zip(d32, d64):
        assert a[2] == b[2]
        assert np.abs(a[0] - b[0]).max() <= 1e-6 and np.abs(a[1] - b[1]).max() <= 1e-6
    dist32 = M.distances(d32[0][1], d32[0][2], [d[1] for d in d32], [d[2] for d in d32])
    dist64 = M.distances64(d64[0][1], d64[0][2], [d[1] for d in d64], [d[2] for d in d64])
    assert np.array_equal(np.isfinite(dist32), np.isfinite(dist64))
    fin = np.isfinite(dist64)
    assert np.abs(dist32[fin] - dist64[fin]).max() <= rings * sectors * 2.0 ** -23


@pytest.mark.parametrize("rings,sectors", [(20, 60), (64, 64), (4, 8)])
def test_a_turned_cloud_gives_its_shift_and_the_start_pose_undoes_it(rings, sectors):
    """(With one ring every non-empty normalised column is the number 1, so the distance is 0 at every shift that overlaps
    and the yaw is not observable: the shapes here have more than one.)"""
    stored = C.cell_centres(5, rings, sectors)
    _, En, emask = M.descriptor(stored, rings, sectors)
    for k in (0, 1, sectors - 1, sectors // 2):
        query = C.turn(stored, k, sectors)
        _, Qn, qmask = M.descriptor(query, rings, sectors)
        out = M.search(Qn, qmask, [En], [emask], [0], 10, 5, 0.2)
        assert out["found"] == 1 and out["shift"] == k and out["score"] < 1e-6, (k, out)
        T0 = M.start_pose(k, sectors)                # the pose of the query in the stored frame: p_stored = T0 p_query
        assert np.abs(query @ T0[:3, :3].T - stored).max() <= 1e-9
        cam = M.start_pose(k, sectors, "-y")
        assert np.abs(C.to_camera(query) @ cam[:3, :3].T - C.to_camera(stored)).max() <= 1e-9


def test_camera_frame_equals_the_permuted_cloud():
    cloud = np.concatenate([C.random_cloud(3, 500), C.edge_rows(20, 60)])
    a = M.descriptor(cloud, up="z")
    b = M.descriptor(C.to_camera(cloud), up="-y")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_edge_rows_lie_where_the_specification_puts_them():
    rings, sectors = 20, 60
    rows = C.edge_rows(rings, sectors)
    keep, ring, sector, h = M.bins(rows, rings, sectors)
    ring_b, dx, dy = M.tables(rings, sectors, C.MAX_RANGE)
    x, y = rows[:, 0], rows[:, 1]
    with np.errstate(all="ignore"):
        r2 = x * x + y * y
    assert (r2 == ring_b[0]).any() and (r2 == ring_b[rings // 2]).any() and (r2 == ring_b[-1]).any()     # rows exactly on a boundary
    assert not keep[~np.isfinite(rows).all(axis=1)].any() and not keep[r2 == 0].any() and not keep[r2 >= ring_b[-1]].any()
    assert (h[np.isfinite(h)] <= 0).any() and not keep[np.isfinite(h) & (h <= 0)].any()
    assert keep[h == np.spacing(np.float32(1.0))].any()                  # one ulp of z above -z_offset
    flat = C.edge_rows(rings, sectors, z_offset=0.0)
    keep0, _, _, h0 = M.bins(flat, rings, sectors, z_offset=0.0)
    assert keep0[h0 == np.nextafter(np.float32(0), np.float32(1))].any() and not keep0[h0 == 0].any()
    on = (np.abs(rows[:, 2] - 1.0) < 1.0) & keep
    assert len(set(sector[on])) >= 5                 # the rows on and beside sector directions fall on both sides


def test_search_rules_in_the_model():
    rings, sectors = 4, 8
    Dn, masks, _ = C.places(7, 3, rings, sectors, 64)
    En, em = np.stack([Dn[0], Dn[1], Dn[1]]), [masks[0], masks[1], masks[1]]
    out = M.search(Dn[1], masks[1], En, em, [0, 1, 2], 30, 5, 0.2)
    assert out["entry"] == 1 and out["found"] == 1                       # two identical entries: the lower one
    ring_only = np.zeros((rings, sectors), dtype=np.float32)
    ring_only[1] = 0.5
    sym = M.normalise(ring_only)
    out = M.search(sym[0], sym[1], [sym[0]], [sym[1]], [0], 30, 5, 0.2)
    assert out["shift"] == 0 and out["found"] == 1                       # a symmetric descriptor: the lowest shift
    empty = np.zeros((rings, sectors), dtype=np.float32)
    out = M.search(empty, 0, En, em, [0, 1, 2], 30, 5, 0.2)
    assert out["found"] == 0 and np.isinf(out["score"]) and out["entry"] == -1
    assert M.search(Dn[1], masks[1], En, em, [25, 26, 27], 30, 5, 0.2)["entry"] == 0      # 25 + 5 == 30 counts, 26 + 5 does not
    assert M.search(Dn[1], masks[1], En, em, [26, 27, 28], 30, 5, 0.2)["entry"] == -1
    pos = np.zeros((31, 3))
    pos[30] = (3.0, 4.0, 0.0)
    assert M.search(Dn[1], masks[1], En, em, [0, 1, 2], 30, 5, 0.2, pos, 5.0)["entry"] == -1     # exactly max_distance: out
    assert M.search(Dn[1], masks[1], En, em, [0, 1, 2], 30, 5, 0.2, pos, np.nextafter(5.0, 6.0))["entry"] == 1
    score = M.search(Dn[0], masks[0], [Dn[1]], [masks[1]], [0], 30, 5, 0.2)["score"]
    assert np.isfinite(score) and score > 0
    assert M.search(Dn[0], masks[0], [Dn[1]], [masks[1]], [0], 30, 5, float(score))["found"] == 0        # score == threshold
    assert M.search(Dn[0], masks[0], [Dn[1]], [masks[1]], [0], 30, 5, float(np.nextafter(score, np.float32(2))))["found"] == 1


@pytest.mark.parametrize("count", C.SEARCH_COUNTS)
def test_search_cases_have_fp64_margins(count):
    """Every decision the GPU tests compare: the winner and its shift lead their runners-up in fp64 by more than 4 x the fp32
    model's own error, the bound the GPU tests would fall back to.  So the GPU tests skip and excuse nothing."""
    c = C.search_case(count)
    _, Qn, qmask = M.descriptor(c["query"], *C.SEARCH_SHAPE)
    entry, shift, err = C.margins(Qn, qmask, c["Dn"], c["masks"])
    assert entry > 4 * err and shift > 4 * err, (entry, shift, err)
    out = M.search(Qn, qmask, c["Dn"], c["masks"], c["frame_ids"], c["f"], C.MIN_ID, 0.2)
    assert (out["entry"], out["shift"], out["found"]) == (c["want"], c["shift"], 1), out


def _revisit_query(stream):
    """The last frame of the whole-chain case against the places that are eligible for it -> (frame ids, d64, d32)."""
    c = C.revisit()
    K = len(c["path"])
    ids = np.arange(K - 1)
    late = ids + C.REVISIT_MIN_ID <= K - 1
    d = c["positions"][ids] - c["positions"][K - 1]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert np.abs(d2[late] - C.REVISIT_MAX_DISTANCE ** 2).min() > 1e-6          # no place sits on the gate: fp64 products of
    ok = M.eligible(ids, K - 1, C.REVISIT_MIN_ID, c["positions"], C.REVISIT_MAX_DISTANCE)     # either order agree on it
    assert ok.sum() >= 3 and ok[:3].all()
    desc = [M.descriptor(c["frames"][k, 0]) for k in ids[ok]]
    q = M.descriptor(c["frames"][K - 1, stream])
    args = (q[1], q[2], [x[1] for x in desc], [x[2] for x in desc])
    return ids[ok], M.distances64(*args), M.distances(*args)


def test_revisit_scene_has_margins():
    """The decisions tests/test_gpu_loop_closure_stream.py asserts for the frame of the return: which place wins, its shift and
    that it is a match, and that the other place is none; each leads in fp64 by more than 4 x the fp32 model's own error, so
    the fp32 order of the kernels cannot decide otherwise."""
    ids, d64, d32 = _revisit_query(0)
    err = float(np.abs(d32.astype(np.float64) - d64)[np.isfinite(d64)].max())
    best = d64.min(axis=1)
    e = int(best.argmin())
    row = np.sort(d64[e])
    # the sensor is turned by +90 degrees, so a landmark lies 15 of the 60 sectors further BACK: shift -15 = 45, T0 = Rz(+90)
    assert ids[e] <= 2 and int(d64[e].argmin()) == 45
    assert np.delete(best, e).min() - best[e] > 4 * err, (best, err)             # over every other place, 0 to 2 included
    assert row[1] - row[0] > 4 * err and 0.2 - best[e] > 4 * err
    assert int(d32.min(axis=1).argmin()) == e and int(d32[e].argmin()) == 45
    _, o64, o32 = _revisit_query(1)
    oerr = float(np.abs(o32.astype(np.float64) - o64)[np.isfinite(o64)].max())
    assert o64.min() - 0.2 > 4 * oerr, (o64.min(), oerr)


# ---- host logic -------------------------------------------------------------------------------------------------------------

def test_host_refusals():
    from pwclonet_pylidarslam_amd import loop_closure as L
    make = lambda **kw: L.ScanContextLoopDetector(**dict(dict(streams=1, num_points=128), **kw))
    for kw in (dict(streams=0), dict(streams=1025), dict(num_points=0), dict(rings=0), dict(rings=65), dict(sectors=7),
               dict(sectors=65), dict(max_range=0.0), dict(max_range=float("inf")), dict(z_offset=float("nan")), dict(up="y"),
               dict(max_keyframes=0), dict(max_loops=0), dict(stride=0), dict(min_id_distance=-1), dict(max_distance=0.0),
               dict(threshold=float("nan")), dict(verify=dict(iterations=3)), dict(verify=dict(iters=0)),
               dict(verify=dict(sigma=0.0)), dict(verify=dict(min_fitness=1.5)), dict(verify=dict(max_mean_cost=-1.0)),
               dict(num_points=63), dict(num_points=16385)):
        with pytest.raises(ValueError, match="ScanContextLoopDetector"):
            make(**kw)
    make(num_points=63, verify=None)                                     # the yaw alone needs no refiner
    det = make()
    cloud = torch.zeros(1, 128, 3)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        det.process(cloud, [0])
    with pytest.raises(ValueError, match="cloud must be float32"):
        det.process(cloud.double(), [0])
    with pytest.raises(ValueError, match="cloud must be float32"):
        det.process(torch.zeros(1, 64, 3), [0])
    with pytest.raises(RuntimeError, match="CPU not supported"):
        L.scan_context(cloud)
    for kw in (dict(rings=0), dict(sectors=4), dict(max_range=-1.0), dict(up="x")):
        with pytest.raises(ValueError, match="scan_context"):
            L.scan_context(cloud, **kw)
    with pytest.raises(ValueError, match="stream=3"):
        det.loops(3)
    assert det.loops() == [] and det.poll() == [] and det.match() is None and det.counts() is None and not det.overflowed()
    assert det.map_bytes() == 1024 * (20 * 60 * 4 + 12 + 128 * 12) + 256 * 160
    with pytest.raises(ValueError, match="num_points"):
        L.ScanContextLoopClosure(0)


def test_tables_are_the_models():
    from pwclonet_pylidarslam_amd import loop_closure as L
    for rings, sectors in C.SHAPES:
        ring_b, sector_d, T0 = L.tables(rings, sectors, C.MAX_RANGE)
        b, dx, dy = M.tables(rings, sectors, C.MAX_RANGE)
        assert np.array_equal(ring_b, b) and np.array_equal(sector_d[:, 0], dx) and np.array_equal(sector_d[:, 1], dy)
        for up in ("z", "-y"):
            T0 = L.tables(rings, sectors, C.MAX_RANGE, up)[2]
            assert max(np.abs(T0[s] - M.start_pose(s, sectors, up)).max() for s in range(sectors)) <= 1e-15


def test_streaming_odometry_refuses_loop_without_backend():
    from pwclonet_pylidarslam_amd.odometry import StreamingOdometry
    with pytest.raises(ValueError, match="loop=.*needs backend="):
        StreamingOdometry(None, streams=1, loop=dict())
    with pytest.raises(ValueError, match="loop=dict\\(streams"):
        StreamingOdometry(None, streams=1, backend=dict(), loop=dict(streams=2))


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
    assert "11. loop detection" in header


# ---- the reference's interface on a stub of the device calls ------------------------------------------------------------------

class _Stub:
    """Stands in for the detector: reports frame 5 as frame 1 again, once."""

    def __init__(self):
        self.calls, self.resets = [], 0

    def reset(self, streams=None):
        self.resets += 1

    def process(self, cloud, frame_ids, trajectory=None, lengths=None):
        self.calls.append((cloud.clone(), list(frame_ids), trajectory[:, 0, :3, 3].clone(), int(lengths[0])))

    def poll(self):
        from pwclonet_pylidarslam_amd.loop_closure import LoopRecord
        if self.calls and self.calls[-1][1] == [5]:
            return [LoopRecord(0, 1, 5, np.eye(4) * 1.0, 0.05, 3, 100, 0.5)]
        return []


def test_reference_interface_on_dicts():
    from pwclonet_pylidarslam_amd.backend import GraphSLAM
    from pwclonet_pylidarslam_amd.loop_closure import ScanContextLoopClosure
    stub = _Stub()
    lc = ScanContextLoopClosure(8, max_frames=16, device="cpu", detector=stub)
    assert lc.pointcloud_key() == "lc_pointcloud" and lc.relative_pose_key() == "lc_relative_pose"
    with pytest.raises(RuntimeError, match="init"):
        lc.process_next_frame({})
    lc.init()
    step = np.eye(4)
    step[0, 3] = 2.0
    for f in range(6):
        d = {"lc_pointcloud": np.full((5 if f == 2 else 11, 3), float(f)), "lc_relative_pose": step}
        lc.process_next_frame(d)
        keys = [k for k in d if k.startswith("se3_loop")]
        assert keys == ([GraphSLAM.se3_loop_closure_constraint(1, 5)] if f == 5 else [])
    assert d[keys[0]][1] is None and d[keys[0]][0].shape == (4, 4)
    assert [c[1] for c in stub.calls] == [[f] for f in range(6)]
    assert stub.calls[2][3] == 5 and stub.calls[3][3] == 8 and stub.calls[2][0].shape == (1, 8, 3)
    assert float(stub.calls[5][2][5, 0]) == 10.0                         # frame 0 at the origin, then five steps of 2 m
    traj = np.tile(np.eye(4), (6, 1, 1))
    traj[:, 1, 3] = np.arange(6)
    lc.update_positions(traj)
    lc.process_next_frame({"lc_pointcloud": np.zeros((8, 3)), "lc_relative_pose": step})
    assert float(stub.calls[6][2][6, 1]) == 5.0 and float(stub.calls[6][2][6, 0]) == 2.0
    lc.process_next_frame({})                                            # a frame without a cloud is passed over
    assert len(stub.calls) == 7
    with pytest.raises(ValueError, match="4, 4"):
        lc.process_next_frame({"lc_pointcloud": np.zeros((8, 3)), "lc_relative_pose": np.eye(3)})


def test_process_and_facade_refusals():
    """The argument checks of ``process`` come before the question where the tensors live, so they are reached here."""
    from pwclonet_pylidarslam_amd import loop_closure as L
    det = L.ScanContextLoopDetector(2, 64, verify=None)
    cloud = torch.zeros(2, 64, 3)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    for kw in (dict(frame_ids=[0]), dict(frame_ids=[0, -1]), dict(frame_ids=[0.5, 1.0]), dict(frame_ids=torch.tensor([0, 1])),
               dict(frame_ids=i32(0, 1, 2)), dict(lengths=torch.tensor([1, 2])), dict(lengths=i32(1)), dict(lengths=[1, 2]),
               dict(trajectory=torch.zeros(3, 2, 4, 4)), dict(trajectory=torch.zeros(3, 1, 4, 4, dtype=torch.float64)),
               dict(trajectory=torch.zeros(0, 2, 4, 4, dtype=torch.float64)), dict(trajectory=np.zeros((3, 2, 4, 4))),
               dict(trajectory=torch.zeros(3, 2, 4, 8, dtype=torch.float64)[..., :4]), dict(active=[1]),
               dict(restart=[0.5, 1.0])):
        with pytest.raises(ValueError, match="ScanContextLoopDetector"):
            det.process(cloud, **dict(dict(frame_ids=[0, 1]), **kw))
    with pytest.raises(ValueError, match="contiguous"):
        det.process(torch.zeros(2, 3, 64).transpose(1, 2), [0, 1])
    with pytest.raises(RuntimeError, match="CPU not supported"):          # everything is in order but the device
        det.process(cloud, i32(0, 1), lengths=i32(64, 64), trajectory=torch.zeros(3, 2, 4, 4, dtype=torch.float64))
    assert det.bufs is None and det.calls == 0                           # refused before any launch or copy
    with pytest.raises(ValueError, match="stream=2"):
        det.reset([2])
    lc = L.ScanContextLoopClosure(8, max_frames=2, device="cpu", detector=_Stub())
    with pytest.raises(RuntimeError, match="init"):
        lc.update_positions(np.eye(4)[None])
    lc.init()
    for bad in (np.eye(4), np.zeros((3, 4, 4)), np.zeros((1, 3, 4))):
        with pytest.raises(ValueError, match="trajectory"):
            lc.update_positions(bad)
    for bad in (np.zeros((0, 3)), np.zeros((5, 2)), np.zeros(5)):
        with pytest.raises(ValueError, match="lc_pointcloud"):
            lc.process_next_frame({"lc_pointcloud": bad})
    short = np.arange(9.0).reshape(3, 3)
    lc.process_next_frame({"lc_pointcloud": short})
    rows = lc.detector().calls[-1][0][0].numpy()
    assert lc.detector().calls[-1][3] == 3 and np.array_equal(rows, short[np.arange(8) % 3].astype(np.float32))   # repeats, no zeros
    lc.process_next_frame({"lc_pointcloud": short})
    with pytest.raises(RuntimeError, match="max_frames=2"):
        lc.process_next_frame({"lc_pointcloud": short})
