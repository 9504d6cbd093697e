"""Keyframe local maps and the refined de-skew prior, the parts that need no GPU: the properties of
the NumPy model of tests/keyframe_model.py, the argument checks of the new keywords, and the ABI's new names."""
import ctypes
import os
import re

import numpy as np
import pytest

import icp_model as model
import keyframe_model as kf
from pwclonet_pylidarslam_amd import _lib, registration
from pwclonet_pylidarslam_amd.odometry import StreamingOdometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the model -------------------------------------------------------------------------------------------------------------

def test_an_empty_map_always_inserts():
    r = np.random.default_rng(1)
    g = kf.Gate(10.0, 90.0)
    g.delta, g.count = kf.small(r, 0.5, 3.0), 7                     # stale words of an earlier sequence
    assert g.step(np.eye(4), any_live=False) == 1 and g.count == 1 and np.array_equal(g.delta, np.eye(4))
    assert g.step(np.eye(4), any_live=True) == 0 and g.count == 1   # and the same frame against a live map does not


def test_the_boundary_is_strict():
    T = model.pose(np.eye(3), [0.125, 0.0, 0.0])
    assert kf.measure(T) == (0.125, 0.0)
    g = kf.Gate(0.125, 0.3)
    assert g.step(T, True) == 0 and np.array_equal(g.delta, T) and g.count == 0
    assert g.step(model.pose(np.eye(3), [2.0 ** -20, 0.0, 0.0]), True) == 1 and np.array_equal(g.delta, np.eye(4))
    z = kf.Gate(0.0, 0.0)                                           # zero thresholds: the identity is not above them
    assert z.step(np.eye(4), True) == 0 and z.step(T, True) == 1


def test_an_idle_stream_leaves_everything_as_it_is():
    r = np.random.default_rng(2)
    g = kf.Gate(0.1, 0.3)
    g.delta, g.count, g.insert = kf.small(r, 0.05, 0.1), 3, 1
    before = g.delta.copy()
    assert g.step(kf.small(r, 5.0, 20.0), any_live=False, active=False) == 0
    assert np.array_equal(g.delta, before) and g.count == 3 and g.insert == 0


def test_sub_threshold_motions_insert_exactly_when_their_product_crosses():
    for trans, deg in ((0.03, 0.0), (0.0, 0.09), (0.02, 0.05)):
        g = kf.Gate(0.1, 0.3)
        acc, inserted = np.eye(4), []
        for k in range(12):                                         # a steady crawl: the same small motion every frame
            T = model.pose(model.rot([0.3, -0.2, 1.0], np.deg2rad(deg)), trans * np.array([0.6, -0.64, 0.48]))
            assert max(kf.measure(T)[0] / 0.1, kf.measure(T)[1] / 0.3) < 1.0       # alone, no frame crosses
            acc = acc @ T
            t, angle = kf.measure(acc)
            want = int(t > 0.1 or angle > 0.3)
            assert g.step(T, True) == want
            inserted.append(want)
            if want:
                acc = np.eye(4)
            assert np.array_equal(g.delta, acc)
        assert 1 <= sum(inserted) < 12 and g.count == sum(inserted)


def test_the_angle_is_the_rotation_angle_at_both_ends():
    for deg in (0.0, 1e-7, 0.3, 45.0, 179.999999, 180.0):
        t, angle = kf.measure(model.pose(model.rot([0.3, -0.2, 1.0], np.deg2rad(deg)), [0.0, 0.0, 0.0]))
        assert t == 0.0 and abs(angle - deg) <= 1e-9 * max(deg, 1e-3)


def test_gated_bookkeeping_moves_the_map_and_keeps_the_slots():
    r = np.random.default_rng(4)
    mp = model.Map(3, 64, 10)
    clouds = r.normal(size=(3, 64, 3)).astype(np.float32)
    nrm = np.zeros((64, 3), dtype=np.float32)
    kf.push(mp, clouds[0], np.eye(4), 1, nrm)
    kf.push(mp, clouds[1], kf.small(r, 0.2, 1.0), 1, nrm)
    A, live, cursor, xyz = mp.A.copy(), mp.live.copy(), mp.cursor, mp.xyz.copy()
    T = kf.small(r, 0.01, 0.01)
    kf.push(mp, clouds[2], T, 0, nrm)
    assert mp.live.tolist() == live.tolist() == [1, 1, 0] and mp.cursor == cursor == 2 and np.array_equal(mp.xyz, xyz)
    assert np.array_equal(mp.A[:2], A[:2] @ T) and np.array_equal(mp.A[2], np.eye(4))
    assert np.allclose(mp.R[:2], np.transpose(mp.A[:2, :3, :3], (0, 2, 1)), atol=1e-15)


def test_pose_row_round_trips_through_every_branch():
    r = np.random.default_rng(5)
    axes = [r.normal(size=3) for _ in range(4)] + [[1, 0.01, 0.01], [0.01, 1, 0.01], [0.01, 0.01, 1]]
    for axis in axes:
        for ang in (0.0, 0.01, 1.0, 3.1):
            T = model.pose(model.rot(axis, ang), r.normal(size=3))
            row = kf.pose_row(T)
            w, x, y, z = row[3:]
            assert w >= 0.0 and abs(np.linalg.norm(row[3:]) - 1.0) < 1e-15 and np.array_equal(row[:3], T[:3, 3])
            R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                          [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                          [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
            assert np.abs(R - T[:3, :3]).max() < 1e-14


# ---- the keywords ----------------------------------------------------------------------------------------------------------

BAD = [dict(trans=-0.1), dict(rot=float("nan")), dict(trans=float("inf")), dict(rot=-1e-9), dict(trans="0.1"),
       dict(trans=0.1, angle=0.3), (0.1, 0.3), 0.1, dict(rot=True)]


@pytest.mark.parametrize("bad", BAD)
def test_keyframe_keyword_is_checked(bad):
    with pytest.raises(ValueError, match="keyframe"):
        registration.IcpRefiner(2, 256, keyframe=bad)


def test_keyframe_keyword_defaults_and_state_before_the_first_call():
    a = registration.IcpRefiner(2, 256)
    b = registration.IcpRefiner(2, 256, keyframe=dict(trans=0.5, rot=0))
    c = registration.IcpRefiner(1, 256, keyframe=dict())
    d = registration.IcpRefiner(2, 256, per_stream=True, keyframe=dict(rot=2.0))
    assert a.keyframe is None and b.keyframe == (0.5, 0.0) and c.keyframe == (0.1, 0.3) and d.keyframe == (0.1, 2.0)
    assert all(x.keyframe_state() is None for x in (a, b, c, d))


def test_streaming_odometry_passes_keyframe_on_and_checks_feedback():
    raw = dict(dataset="kitti360", capacity=4096)
    kfd = dict(trans=0.1, rot=0.3)
    on = StreamingOdometry(None, streams=2, refine=dict(map_size=2, keyframe=kfd))
    assert on._refine_cfg == dict(map_size=2, keyframe=kfd) and on._feedback is False
    per = StreamingOdometry(None, streams=2, per_stream=True, refine=dict(per_stream=True, keyframe=kfd))
    assert per._refine_cfg["keyframe"] == kfd
    image = dict(kind="projective", height=16, width=64)
    with pytest.raises(ValueError, match="keyframe"):                       # the projective refiner has no gate
        StreamingOdometry(None, streams=2, num_points=256, sweeps=raw, refine=dict(image, keyframe=kfd))
    pf = StreamingOdometry(None, streams=2, num_points=256, sweeps=dict(raw, deskew=True), refine=dict(image, feedback=True))
    assert pf._feedback is True and pf._refine_kind == "projective" and pf._refine_cfg == dict(height=16, width=64)
    with pytest.raises(ValueError, match="feedback"):
        StreamingOdometry(None, streams=2, num_points=256, sweeps=raw, refine=dict(image, feedback=True))
    for sweeps in (None, raw, dict(raw, deskew=False)):
        with pytest.raises(ValueError, match="feedback"):
            StreamingOdometry(None, streams=2, num_points=256, sweeps=sweeps, refine=dict(map_size=2, feedback=True))
    with pytest.raises(ValueError, match="feedback"):
        StreamingOdometry(None, streams=2, refine=dict(map_size=2, feedback=1))
    fb = StreamingOdometry(None, streams=2, num_points=256, sweeps=dict(raw, deskew=True),
                           refine=dict(map_size=2, feedback=True))
    off = StreamingOdometry(None, streams=2, num_points=256, sweeps=dict(raw, deskew=True),
                            refine=dict(map_size=2, feedback=False))
    assert fb._feedback is True and off._feedback is False and fb._refine_cfg == off._refine_cfg == dict(map_size=2)


def test_gate_op_checks_its_arguments_before_any_launch():
    import torch
    T, live = torch.zeros(2, 4, 4, dtype=torch.float64), torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="trans"):
        registration.keyframe_gate(T, T.clone(), live, -1.0, 0.3)
    with pytest.raises(ValueError, match="rot"):
        registration.keyframe_gate(T, T.clone(), live, 0.1, float("nan"))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        registration.keyframe_gate(T, T.clone(), live, 0.1, 0.3)


# ---- declarations ----------------------------------------------------------------------------------------------------------

NEW = [("keyframe_gate_kernel_wrapper", 10), ("keyframe_icp_push_kernel_wrapper", 16),
       ("stream_motion_from_refined_kernel_wrapper", 5)]


@pytest.mark.parametrize("name, arity", NEW)
def test_new_symbols_are_declared_with_the_header_arity(name, arity):
    args, res = _lib.SIGNATURES[name]
    with open(os.path.join(ROOT, "include", "pwclo_ops.h")) as f:
        header = f.read()
    m = re.search(r"void\s+%s\s*\(([^)]*)\)\s*;" % name, header)
    assert m is not None, "%s is not declared in include/pwclo_ops.h" % name
    assert res is None
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(args) == len(params) == arity
    for p, a in zip(params, args):
        want = _lib._F if "*" in p else ctypes.c_float if p.startswith("float") else \
            ctypes.c_double if p.startswith("double") else _lib._i
        assert a is want, (name, p, a)
    assert hasattr(_lib.load(), name)


def test_the_gated_pushes_extend_the_plain_ones_and_the_version_stays():
    sig = lambda n: _lib.SIGNATURES[n][0]
    assert sig("keyframe_icp_push_kernel_wrapper")[:-1] == sig("icp_map_push_masked_kernel_wrapper")
    with open(os.path.join(ROOT, "include", "pwclo_ops.h")) as f:
        header = f.read()
    assert set(re.findall(r"\b(keyframe_\w+)\s*\(", header)) == {n for n, _ in NEW[:2]}
    assert _lib.load().pwclo_abi_version() == 1                                  # additions only
