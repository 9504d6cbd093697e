"""GPU tests of the loop-detection chain with the translation search: a return that passes 2 m beside
the start, twice the verifying refiner's pairing radius, is refused without ``translation=`` and closed with it; the
decisions are those tests/test_elevation_cpu.py::test_offset_revisit_scene_has_margins takes on the model chain."""
import functools

import numpy as np
import pytest
import torch

import elevation_cases as EC
from oracle import params
from pwclonet_pylidarslam_amd.loop_closure import ScanContextLoopDetector
from pwclonet_pylidarslam_amd.odometry import StreamingOdometry
from pwclonet_pylidarslam_amd.pose_graph import PoseGraph
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet
from pwclonet_pylidarslam_amd.registration import IcpRefiner

pytestmark = pytest.mark.gpu
N = EC.OFFSET_N
STATE = ("db_desc", "db_mask", "db_frame", "db_cloud", "count", "epoch", "overflow", "nlog", "log_i", "log_T", "log_c",
         "log_overflow", "match", "match_score", "accepted", "ei_img", "ei_occ", "ei_A", "ei_record", "T1")
LOOP = dict(min_id_distance=EC.OFFSET_MIN_ID, max_distance=EC.OFFSET_MAX_DISTANCE, max_keyframes=64,
            threshold=EC.OFFSET_THRESHOLD, verify=dict(EC.OFFSET_VERIFY, **EC.OFFSET_ACCEPT))


def _error(T, truth):
    d = np.linalg.inv(truth) @ T
    angle = np.arccos(np.clip((np.trace(d[:3, :3]) - 1.0) / 2.0, -1.0, 1.0))
    return float(np.linalg.norm(d[:3, 3])), float(angle)


def _fixed_point(cuda, stored, query, truth):
    """What the verifying refiner returns when it starts from the true pose on the same two clouds."""
    ref = IcpRefiner(1, N, map_size=1, graph=False, **EC.OFFSET_VERIFY)
    ref.register(torch.from_numpy(stored[None]).to(cuda), torch.eye(4, dtype=torch.float64, device=cuda)[None])
    return ref.register(torch.from_numpy(query[None]).to(cuda), torch.from_numpy(truth[None]).to(cuda))[0].cpu().numpy()


def _held_to_the_yardstick(cuda, c, recs):
    """Exactly the return is logged, and its pose lies no further from the truth than 4 x the refiner's own fixed point."""
    path, frames = c["path"], c["frames"]
    K = len(path)
    assert [(q.stream, q.i, q.j, q.shift) for q in recs] == [(0, 0, K - 1, 57)], recs
    q = recs[0]
    truth = np.linalg.inv(path[q.i]) @ path[q.j]
    yard = _error(_fixed_point(cuda, frames[q.i, 0], frames[q.j, 0], truth), truth)
    got = _error(q.T, truth)
    print("record", q.i, q.j, q.shift, q.score, q.pairs, q.cost / q.pairs, "error (m, rad)", got, "fixed point", yard, "ratios",
          got[0] / yard[0], got[1] / yard[1])
    assert got[0] <= 4 * yard[0] and got[1] <= 4 * yard[1], q
    assert q.pairs >= EC.OFFSET_ACCEPT["min_fitness"] * N


def test_offset_revisit_needs_the_translation_search(cuda):
    """The pose graph gets the drifted chain frame by frame and its vertices are the positions of the distance gate.  (a)
    Without ``translation=`` the log stays empty: the return is matched and refused.  (b) With it the return is logged, and
    nothing else.  Eager equals replay, the images, scores and seeds included.  Measured: the logged pose 1.00 x the fixed
    point; see DESIGN.md section 26."""
    c = EC.offset_revisit()
    path, frames, chain = c["path"], c["frames"], c["chain"]
    K = len(path)
    plain = ScanContextLoopDetector(1, N, device=cuda, **LOOP)
    det = ScanContextLoopDetector(1, N, device=cuda, translation=EC.OFFSET_TRANSLATION, **LOOP)
    eager = ScanContextLoopDetector(1, N, device=cuda, graph=False, translation=EC.OFFSET_TRANSLATION, **LOOP)
    pg = PoseGraph(1, max_poses=64, max_loops=8, max_absolute=2, iters=20, device=cuda)
    for k in range(K):
        if k:
            pg.append(torch.from_numpy(chain[k][None]).to(cuda))
        for d in (plain, det, eager):
            d.process(torch.from_numpy(frames[k]).to(cuda), [k], trajectory=pg.bufs["X"])
    assert det.captures == 1 and eager.captures == 0 and not det.overflowed() and det.counts().tolist() == [K]
    for name in STATE:
        assert torch.equal(det.bufs[name], eager.bufs[name]), name
    for name in ("status", "pairs", "cost", "T"):
        assert torch.equal(det.refiner().bufs[name], eager.refiner().bufs[name]), name
    # (a) matched, verified from T0, refused
    m = plain.match()
    assert (int(m["found"][0]), int(m["frame_i"][0]), int(m["shift"][0]), int(m["accepted"][0])) == (1, 0, 57, 0)
    print("without translation: pairs", int(plain.refiner().bufs["pairs"][0]), "cost", float(plain.refiner().bufs["cost"][0]))
    assert plain.loops() == [] and plain.seed() is None
    # (b) the same match, seeded and accepted
    for name in ("match", "match_score"):
        assert torch.equal(det.bufs[name], plain.bufs[name]), name
    seed = det.seed()
    got = tuple(int(seed[k][0]) for k in ("found", "k", "a", "b"))
    print("seed", got, "A", int(seed["A"][0]), "cells", int(seed["occ_q"][0]), int(seed["occ_e"][0]))
    assert got == (1, 5, 0, -2)
    recs = det.loops()
    _held_to_the_yardstick(cuda, c, recs)
    end = lambda X: _error(np.linalg.inv(X[0]) @ X[K - 1], np.linalg.inv(path[0]) @ path[K - 1])[0]
    before = end(pg.poses(0).cpu().numpy())
    added = det.hand_over(pg, optimize=True)
    after = end(pg.poses(0).cpu().numpy())
    print("end-to-start error: drifted %.4f, optimised %.4f" % (before, after))
    assert len(added) == 1 and det.dropped == [] and after < before


@functools.lru_cache(maxsize=None)
def _net(dev):
    """The suite's synthetic weights with every pose head's last layer set to "no motion" (tests/test_gpu_icp_masked.py)."""
    net = PWCLONet(dict(num_input_channels=3, sequence_len=2, device=str(dev), scalar_last=False, log_mode="none",
                        fused="auto"))
    sd = net.state_dict()
    params.fill_state_dict(sd)
    for key, v in sd.items():
        if key.endswith(("conv1d_q.conv.weight", "conv1d_t.conv.weight", "conv1d_t.conv.bias")):
            v.zero_()
        elif key.endswith("conv1d_q.conv.bias"):
            v.copy_(torch.tensor([1.0, 0.0, 0.0, 0.0]))
    net = net.to(dev).eval()
    net.prepare_fused()
    return net


def test_streaming_odometry_passes_the_keyword_and_closes_the_return(cuda):
    """The step's clouds through ``StreamingOdometry(backend=..., loop=dict(translation=...))``.  The network says "no
    motion", so the backend's chain ends at the start, 2 m and 14 degrees from where the sensor is: ``poll_loops(optimize=True)``
    must lower the end-to-start error (measured: 2.015 m before, 0.690 m after: one loop edge against 39 odometry edges that
    all say "no motion"); without ``translation=`` nothing is logged and nothing moves."""
    c = EC.offset_revisit()
    path, frames = c["path"], c["frames"]
    K = len(path)
    net = _net(cuda)
    backend = dict(source="network", max_loops=4, iters=20)
    outcomes = {}
    for name, loop in (("plain", dict(LOOP)), ("seeded", dict(LOOP, translation=EC.OFFSET_TRANSLATION))):
        so = StreamingOdometry(net, streams=1, max_frames=64, backend=dict(backend), loop=loop)
        with torch.no_grad():
            for k in range(K):
                so.step(torch.from_numpy(frames[k]).to(cuda))
        det = so.loop_detector()
        assert (det.translation is None) == (name == "plain") and det.counts().tolist() == [K]
        end = lambda: _error((lambda X: np.linalg.inv(X[0]) @ X[K - 1])(so.backend().poses(0).cpu().numpy()),
                             np.linalg.inv(path[0]) @ path[K - 1])[0]
        before = end()
        recs = so.poll_loops(optimize=True)
        outcomes[name] = (recs, before, end())
    assert outcomes["plain"][0] == [] and outcomes["plain"][1] == outcomes["plain"][2]
    recs, before, after = outcomes["seeded"]
    _held_to_the_yardstick(cuda, c, recs)
    print("end-to-start error: chain %.4f, optimised %.4f" % (before, after))
    assert before > 1.5 and after < before
