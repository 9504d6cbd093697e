"""Masked (per-stream) point-to-plane registration, the parts that need no GPU: the host model of
tests/icp_mask_model.py keeps the three-case rule, the shared schedule gives under the model alone what
tests/test_gpu_icp_masked.py relies on, the host-side argument checks, and the ABI's new names."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import icp_mask_model as masked
import icp_model as model
from pwclonet_pylidarslam_amd import _lib, registration, stream_masks
from pwclonet_pylidarslam_amd.odometry import StreamingOdometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_schedule_is_the_issues():
    calls = masked.schedule()
    assert [c["active"].tolist() for c in calls] == [[1, 1, 0], [1, 0, 1], [1, 1, 1], [0, 1, 1], [1, 1, 1], [1, 1, 1]]
    assert [c["restart"].tolist() for c in calls] == [[0, 0, 0]] * 3 + [[0, 0, 1]] + [[0, 0, 0]] * 2
    assert [c["reset"] for c in calls] == [[], [], [], [], [], [1]]
    assert [c["frame"].tolist() for c in calls] == [[0, 0, -1], [1, -1, 0], [2, 1, 1], [-1, 2, 2], [3, 3, 3], [4, 4, 4]]
    assert [c["primes"].tolist() for c in calls] == [[True, True, False], [False, False, True], [False] * 3,
                                                     [False, False, True], [False] * 3, [False, True, False]]
    for c in calls:                                               # idle rows are poison: nothing may read them
        assert np.isnan(c["cloud"][c["active"] == 0]).all() and np.isfinite(c["cloud"][c["active"] != 0]).all()


def test_model_keeps_the_three_case_rule_and_registers_every_pair():
    """What the GPU test relies on, under the model alone: every pair call keeps more than 0.9 n pairs and freezes for no
    bad reason at iters = 6; every priming call returns init; an idle call leaves the Map object untouched."""
    calls = masked.schedule()
    maps = masked.MaskedMaps(masked.S, masked.M, masked.N)
    pairs = 0
    for c, call in enumerate(calls):
        maps.reset(call["reset"])
        before = list(maps.maps)
        state = [(mp.A.copy(), mp.R.copy(), mp.live.copy(), mp.cursor, mp.xyz.copy(), mp.normals.copy()) for mp in before]
        out = maps.register(call["cloud"], call["init"], call["active"], call["restart"], iters=6)
        for s in range(masked.S):
            o, mp = out[s], maps.maps[s]
            if not call["active"][s]:
                assert mp is before[s] and all(np.array_equal(a, b) for a, b in zip(
                    state[s], (mp.A, mp.R, mp.live, mp.cursor, mp.xyz, mp.normals)))
                assert o["status"] == masked.IDLE and o["iterations"] == 0 and o["pairs"] == 0
                assert np.array_equal(o["T"], call["init"][s])
            elif call["primes"][s]:
                assert o["status"] == model.FEW_PAIRS and o["iterations"] == 1 and o["pairs"] == 0
                assert np.array_equal(o["T"], call["init"][s]) and np.array_equal(o["T"], np.eye(4))
                assert mp.live.tolist() == [1, 0] and mp.cursor == 1
                assert (mp is not before[s]) == (bool(call["restart"][s]) or s in call["reset"])
            else:
                pairs += 1
                assert mp is before[s]
                assert not o["status"] & (model.FEW_PAIRS | model.BAD_PIVOT), (c, s, o["status"])
                assert o["pairs"] > 0.9 * masked.N, (c, s, o["pairs"])
                e0, e1 = model.pose_error(call["init"][s], call["gt"][s]), model.pose_error(o["T"], call["gt"][s])
                assert e1 <= 0.1 * e0, (c, s, e0, e1)
    assert pairs == 10


def test_mask_argument_rules():
    ref = registration.IcpRefiner(3, 256, map_size=2, per_stream=True)
    lock = registration.IcpRefiner(3, 256, map_size=2)
    assert ref.per_stream and not lock.per_stream and registration.IDLE == masked.IDLE == 8
    cloud, init = torch.zeros(3, 256, 3), torch.eye(4, dtype=torch.float64).repeat(3, 1, 1)
    for bad in ([1, 1], [[1, 1, 1]], [1.0, 0.0, 1.0], np.ones((4,), dtype=bool), torch.ones(3), torch.ones(2, dtype=torch.int32)):
        for key in ("active", "restart"):
            with pytest.raises(ValueError, match=key):            # before any launch: the CPU tensors are not reached
                ref.register(cloud, init, **{key: bad})
    for key in ("active", "restart"):
        with pytest.raises(ValueError, match="per_stream"):
            lock.register(cloud, init, **{key: [1, 1, 1]})
    for good in ([1, 0, 1], [True, False, True], np.array([1, 0, 2]), torch.tensor([True, False, False])):
        with pytest.raises(RuntimeError, match="CPU not supported"):
            ref.register(cloud, init, active=good, restart=good)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ref.register(cloud, init)
    with pytest.raises(ValueError, match="trace"):
        ref.register(cloud, init, active=[1, 1, 1], trace=True)
    assert ref.bufs is None and ref.calls == 0
    ref.reset(streams=[1])                                        # before the first call: nothing to arm
    ref.reset()
    with pytest.raises(ValueError, match="outside"):
        ref.reset(streams=[3])
    with pytest.raises(RuntimeError, match="CPU not supported"):
        registration.queries(torch.zeros(1, 2, 4, 4, dtype=torch.float64), torch.zeros(1, 10, 3),
                             active=torch.ones(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="A must be"):
        registration.begin(None, None, None, None, None, None)
    with pytest.raises(ValueError, match="map_xyz"):
        registration.map_push(*[None] * 11)


def test_the_shared_mask_helper_accepts_and_refuses_each_form_once():
    f = stream_masks.stream_mask
    for good in ([1, 0, 2], [True, False, True], np.array([1, 0, 1], dtype=np.uint8), torch.tensor([True, False, True]),
                 torch.tensor([3, 0, 1])):
        got = f(good, 3, "active", "Owner")
        assert got.dtype == torch.int32 and got.tolist() == [1, 0, 1] and not got.is_cuda
    assert f([2, 0], 3, "streams", "Owner", indices=True).tolist() == [1, 0, 1]             # integers: stream indices
    assert f([], 3, "streams", "Owner", indices=True).tolist() == [0, 0, 0]
    assert f([False, True, False], 3, "streams", "Owner", indices=True).tolist() == [0, 1, 0]
    assert f(torch.tensor([0, 0]), 3, "streams", "Owner", indices=True).tolist() == [1, 0, 0]
    for bad in ([1, 0], [[1, 0, 1]], [1.0, 0.0, 1.0], torch.ones(3), np.ones((4,), dtype=bool), "101"):
        with pytest.raises(ValueError, match=r"^Owner: active must be a \(3,\) bool or integer mask"):
            f(bad, 3, "active", "Owner")
    for bad in ([3], [-1], np.array([0, 5])):
        with pytest.raises(ValueError, match=r"^Owner: streams .* outside \[0, 3\)"):
            f(bad, 3, "streams", "Owner", indices=True)
    for bad in ([True, False], [0.0], [[0]]):
        with pytest.raises(ValueError, match=r"^Owner: streams must be a \(3,\) bool or integer mask"):
            f(bad, 3, "streams", "Owner", indices=True)
    # idle rows start as copies of the first active row; the caller's tensors stay as they are
    x = torch.arange(12.0).view(3, 4)
    host, y, none = stream_masks.seed_idle_rows(torch.tensor([0, 1, 0], dtype=torch.int32), 3, "Owner", x, None)
    assert host.tolist() == [False, True, False] and none is None and y is not x
    assert y.tolist() == [x[1].tolist()] * 3 and x[0].tolist() == [0.0, 1.0, 2.0, 3.0]
    host, y = stream_masks.seed_idle_rows(None, 3, "Owner", x)
    assert host.all() and y is x
    with pytest.raises(ValueError, match="^Owner: .*at least one active stream"):
        stream_masks.seed_idle_rows(torch.zeros(3, dtype=torch.int32), 3, "Owner", x)
    # the two words
    a, r = torch.zeros(3, dtype=torch.int32), torch.ones(3, dtype=torch.int32)
    stream_masks.load_words(a, r, None, None)
    assert a.tolist() == [1, 1, 1] and r.tolist() == [0, 0, 0]
    stream_masks.load_words(a, r, torch.tensor([0, 1, 0], dtype=torch.int32), torch.tensor([0, 1, 1], dtype=torch.int32))
    assert a.tolist() == [0, 1, 0] and r.tolist() == [0, 1, 1]


def test_streaming_constructor_rules():
    with pytest.raises(ValueError, match=r"per_stream.*refine=dict\(\.\.\., per_stream=True\)"):
        StreamingOdometry(None, streams=2, per_stream=True, refine=dict(map_size=2))
    with pytest.raises(ValueError, match="per_stream"):
        StreamingOdometry(None, streams=2, per_stream=True, refine=dict(map_size=2, per_stream=False))
    with pytest.raises(ValueError, match="per_stream"):
        StreamingOdometry(None, streams=2, refine=dict(map_size=2, per_stream=True))
    on = StreamingOdometry(None, streams=2, per_stream=True, refine=dict(map_size=2, per_stream=True))
    assert on._refine_cfg == dict(map_size=2, per_stream=True) and on.refiner() is None
    with pytest.raises(ValueError, match="stream=i"):
        on.refined_relative_poses()
    with pytest.raises(ValueError, match="stream=i"):
        on.refined_trajectory()
    assert on.refined_relative_poses(stream=1).shape == (0, 4, 4) and on.refined_trajectory(stream=0).shape == (0, 4, 4)
    with pytest.raises(ValueError, match="outside"):
        on.refined_relative_poses(stream=2)
    lock = StreamingOdometry(None, streams=2, refine=dict(map_size=2))
    assert lock.refined_relative_poses().shape == (0, 2, 4, 4) and lock.refined_trajectory().shape == (0, 2, 4, 4)
    for view in (lock.refined_relative_poses, lock.refined_trajectory):
        with pytest.raises(ValueError, match="per_stream"):
            view(stream=0)
    plain = StreamingOdometry(None, streams=2, per_stream=True)
    for view in (plain.refined_relative_poses, plain.refined_trajectory):
        with pytest.raises(RuntimeError, match="refine="):
            view(stream=0)


# ---- declarations ----------------------------------------------------------------------------------------------------------

NEW = [("icp_begin_kernel_wrapper", 9), ("icp_queries_masked_kernel_wrapper", 8), ("icp_accumulate_masked_kernel_wrapper", 16),
       ("icp_solve_masked_kernel_wrapper", 15), ("icp_map_push_masked_kernel_wrapper", 15),
       ("stream_record_refined_kernel_wrapper", 8)]
OLD = {"icp_queries_masked_kernel_wrapper": "icp_queries_kernel_wrapper",
       "icp_accumulate_masked_kernel_wrapper": "icp_accumulate_kernel_wrapper",
       "icp_solve_masked_kernel_wrapper": "icp_solve_kernel_wrapper",
       "icp_map_push_masked_kernel_wrapper": "icp_map_push_kernel_wrapper"}


def _declared(name):
    """The parameter list of ``name`` in the header.  The masked icp names are followed by an empty comment there (the
    header says why), which C reads as white space."""
    with open(os.path.join(ROOT, "include", "pwclo_ops.h")) as f:
        header = f.read()
    m = re.search(r"void\s+%s\s*(?:/\*\*/\s*)?\(([^)]*)\)\s*;" % name, header)
    assert m is not None, "%s is not declared in include/pwclo_ops.h" % name
    return [p.strip() for p in m.group(1).split(",")]


@pytest.mark.parametrize("name, arity", NEW)
def test_new_symbols_are_declared_with_the_header_arity(name, arity):
    args, res = _lib.SIGNATURES[name]
    params = _declared(name)
    assert res is None and len(args) == len(params) == arity
    for p, a in zip(params, args):
        want = _lib._F if "*" in p else ctypes.c_float if p.startswith("float") else \
            ctypes.c_double if p.startswith("double") else _lib._i
        assert a is want, (name, p, a)
    assert hasattr(_lib.load(), name)
    if name in OLD:                                               # the old argument list plus `const int *active`
        assert params[:-1] == _declared(OLD[name]) and params[-1] == "const int *active"
        assert _lib.SIGNATURES[OLD[name]][0] == args[:-1]


def test_status_bits_and_version():
    with open(os.path.join(ROOT, "pwclonet_pylidarslam_amd", "csrc", "icp.hpp")) as f:
        hpp = f.read()
    assert "ICP_IDLE = 8" in hpp and "ICP_CONVERGED = 1, ICP_FEW_PAIRS = 2, ICP_BAD_PIVOT = 4" in hpp
    assert _lib.load().pwclo_abi_version() == 1                   # additions only
