"""Point-to-plane registration, the parts that need no GPU: the NumPy model of tests/icp_model.py
converges on its own scenes, the inputs of tests/test_gpu_icp.py satisfy under the model alone what those tests rely on,
the host-side argument checks, and the ABI's new names."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import icp_model as model
from pwclonet_pylidarslam_amd import _lib, registration
from pwclonet_pylidarslam_amd.odometry import PWCLONetOdometry, StreamingOdometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _registered(walls, seed=3, n=1024):
    clouds, gt = model.room(seed, 3, n, walls_only=walls)
    mp = model.Map(2, n, 10)
    mp.push(clouds[0], np.eye(4))
    init = model.perturbed(gt[1])
    T, status, steps = model.register(mp, clouds[1], init)
    return clouds, gt, init, T, status, steps, mp


def test_model_converges_on_the_room_from_2_degrees_and_30_cm():
    clouds, gt, init, T, status, steps, mp = _registered(False)
    e0, e1 = model.pose_error(init, gt[1]), model.pose_error(T, gt[1])
    assert 0.3 < e0 < 0.4                                        # 0.3 m + 2 degrees
    assert e1 <= 0.1 * e0 and e1 < 0.03, (e0, e1)
    assert status == model.CONVERGED and steps[-1]["row"][model.PAIRS] >= 0.9 * 1024
    norms = [np.linalg.norm(s["delta"]) for s in steps]
    assert norms[2] < 0.1 * norms[0]
    # what the teacher-forced GPU test relies on: the damped system is well conditioned at every iteration, so sums that
    # differ by fp64 rounding (n eps) give steps that agree far inside 1e-10
    for s in steps:
        if s["row"][model.SW] > 0:
            assert np.linalg.cond(model.system(s["row"], 1e-6)[0]) < 1e3
    assert mp.live.tolist() == [1, 1] and mp.cursor == 0        # the push after the registration


def test_room_has_three_mutually_non_parallel_planes_and_walls_only_has_two():
    for walls, want in ((False, 3), (True, 2)):
        clouds, _ = model.room(3, 2, 1024, walls_only=walls)
        nrm = model.normals(clouds[0], 10)[0]
        flat = nrm[model.normals(clouds[0], 10)[2] > 0.5]           # clean planar neighbourhoods
        axes = np.abs(flat).argmax(axis=1)
        share = np.bincount(axes, minlength=3) / len(axes)
        assert int((share > 0.05).sum()) == want, share


def test_walls_only_leaves_the_vertical_weak_and_damping_keeps_an_exact_null_direction():
    clouds, gt, init, T, status, steps, _ = _registered(True)
    H, _ = model.system(steps[0]["row"], 0.0)
    assert H[5, 5] < 1e-2 * min(H[3, 3], H[4, 4])               # translation along z: noise in the normals only
    row = model.planted_rows(flat=True)
    H, g = model.system(row, 0.0)
    assert not H[5].any() and not H[:, 5].any() and g[5] == 0.0
    out = model.solve(row, np.eye(4), 0, 0, 1e-6, 1e-4, 64)
    assert out["status"] == 0 and out["delta"][5] == 0.0 and np.abs(out["delta"][:5]).min() > 0.0
    assert model.solve(row, np.eye(4), 0, 0, 0.0, 1e-4, 64)["status"] == model.BAD_PIVOT
    assert model.solve(model.planted_rows(pairs=10), np.eye(4), 0, 0, 1e-6, 1e-4, 64)["status"] == model.FEW_PAIRS


@pytest.mark.parametrize("b, n, k", model.NORMAL_SHAPES)
def test_normal_inputs_stay_within_the_gap_cap(b, n, k):
    """The GPU test may leave out points whose relative eigen-gap is below 1e-3, up to 2 % of a cloud: the inputs it
    uses need no more than that, and none of their points is degenerate."""
    x = model.normals_cloud(b, n)
    for c in range(b):
        nrm, val, gap = model.normals(x[c], k)
        assert (gap < model.GAP_MIN).mean() <= model.GAP_CAP
        assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-12)
        assert (np.einsum("ni,ni->n", nrm, x[c].astype(np.float64)) <= 0.0).all()


def test_model_normals_of_degenerate_clouds_are_zero():
    line = np.zeros((64, 3), dtype=np.float32)
    line[:, 0] = np.arange(64) * 0.5
    assert not model.normals(line, 10)[0].any()
    dup = np.tile(np.array([[1.0, 2.0, 3.0]], dtype=np.float32), (64, 1))
    assert not model.normals(dup, 10)[0].any()


def test_planted_inputs_hold_every_case():
    c = model.planted()
    slot0, ok0 = model.choose(c["dist"][0], c["live"][0], c["max_dist"])
    assert (slot0[::5][ok0[::5]] == 0).all() and ok0[::5].any()                   # ties go to the lower slot
    slot1, ok1 = model.choose(c["dist"][1], c["live"][1], c["max_dist"])
    assert not (slot1 == 1).any() and ok1[1::7].all()                             # dead slot unused; dist == max_dist kept
    assert (c["dist"][1, 0, 1::7] == np.float32(c["max_dist"])).all()
    assert not model.choose(c["dist"][2], c["live"][2], c["max_dist"])[1].any()   # stream 2: nothing survives
    for s in range(3):
        row, mag = model.accumulate(c["p"][s], c["q"][s], c["idx"][s], c["dist"][s], c["map_xyz"][s], c["map_normals"][s],
                                    c["live"][s], c["R"][s], c["T"][s], c["sigma"], c["max_dist"])
        assert np.isfinite(row).all()
        assert (row[model.PAIRS] == 0) == (s == 2)
    y = c["map_xyz"][0, 0][c["idx"][0, 0]].astype(np.float64)
    r = np.einsum("ni,ni->n", c["map_normals"][0, 0][c["idx"][0, 0]].astype(np.float64), c["q"][0, 0] - y)
    assert (np.abs(r) < c["sigma"]).sum() > 20 and (np.abs(r) > c["sigma"]).sum() > 20
    assert c["p"].shape[1] % 64 != 0 and registration.groups(c["p"].shape[1]) > 1


def test_model_registers_the_walls_only_sequences_from_no_motion():
    """What the streaming GPU test relies on: from the guess "no motion", with its settings, the model finds pairs for
    every point and lands within 10 cm of ``synthetic.kitti_like_sequence``'s ground truth, most of it vertical."""
    from pwclonet_pylidarslam_amd import synthetic
    n = 1024
    for seed in (31, 32):
        pcs, q, t = synthetic.kitti_like_sequence(seed, n, 4)
        mp = model.Map(2, n, 10)
        for k in range(4):
            T, status, steps = model.register(mp, pcs[k, :, :3], np.eye(4), iters=8, max_dist=2.0)
            if k == 0:
                assert status == model.FEW_PAIRS and np.array_equal(T, np.eye(4))
                continue
            gt = model.pose(model.rot([0, -1, 0], 2 * np.arctan2(-q[k - 1][2], q[k - 1][0])), t[k - 1].astype(np.float64))
            assert status in (0, model.CONVERGED) and steps[-1]["row"][model.PAIRS] == n
            assert model.pose_error(np.eye(4), gt) > 0.5 and model.pose_error(T, gt) < 0.1
            assert np.linalg.norm(T[:3, 3]) > 0.3


def test_huber_weights_are_the_references():
    r = np.array([0.0, 1e-5, 0.49, 0.5, 2.0, -2.0])
    w2 = model.huber_w2(r, 0.5)
    assert w2[:3].tolist() == [1.0, 1.0, 1.0]
    assert np.allclose(w2[3:], [(2 * 0.5 * 0.5 - 0.25) / 0.25, (2.0 - 0.25) / 4.0, (2.0 - 0.25) / 4.0])


def test_host_side_argument_checks():
    ok = dict(streams=2, num_points=256)
    for bad, match in ((dict(streams=0), "streams"), (dict(num_points=63), "num_points"), (dict(num_points=16385), "num_points"),
                       (dict(map_size=0), "map_size"), (dict(map_size=65), "map_size"), (dict(iters=0), "iters"),
                       (dict(sigma=0.0), "sigma"), (dict(max_dist=-1.0), "max_dist"), (dict(k_normals=64), "k_normals"),
                       (dict(k_normals=0), "k_normals"), (dict(damping=-1e-6), "damping"),
                       (dict(threshold_delta_pose=-1.0), "threshold"), (dict(min_pairs=0), "min_pairs")):
        with pytest.raises(ValueError, match=match):
            registration.IcpRefiner(**dict(ok, **bad))
    ref = registration.IcpRefiner(**ok)
    assert ref.status() is None and ref.diagnostics() is None and ref.map_state() is None
    cloud, init = torch.zeros(2, 256, 3), torch.eye(4, dtype=torch.float64).repeat(2, 1, 1)
    with pytest.raises(ValueError, match="cloud"):
        ref.register(torch.zeros(2, 255, 3), init)
    with pytest.raises(ValueError, match="init"):
        ref.register(cloud, init.float())
    with pytest.raises(ValueError, match="init"):
        ref.register(cloud, torch.zeros(2, 7, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        ref.register(cloud, init)
    with pytest.raises(ValueError, match="trace"):
        ref.register(cloud, init, trace=True)
    with pytest.raises(ValueError, match="outside"):
        ref.reset(streams=[2])
    with pytest.raises(ValueError, match="mask"):
        ref.reset(streams=np.array([True]))
    ref.reset(streams=[1])
    ref.reset()
    with pytest.raises(ValueError, match="n=63"):
        registration.normals(torch.zeros(1, 63, 3))
    with pytest.raises(ValueError, match="k=64"):
        registration.normals(torch.zeros(1, 128, 3), k=64)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        registration.normals(torch.zeros(1, 128, 3))
    with pytest.raises(RuntimeError, match="CPU not supported"):
        registration.queries(torch.zeros(1, 2, 4, 4, dtype=torch.float64), torch.zeros(1, 10, 3))
    with pytest.raises(ValueError, match="sigma"):
        registration.accumulate(None, torch.zeros(1, 1, 8, 3), None, None, None, None, None, None, None, sigma=0.0)


def test_refine_is_opt_in_and_refuses_per_stream_mode():
    with pytest.raises(ValueError, match="per_stream"):
        StreamingOdometry(None, streams=2, per_stream=True, refine=dict(map_size=2))
    plain = StreamingOdometry(None, streams=2)
    assert plain._refine_cfg is None and plain.refiner() is None
    with pytest.raises(RuntimeError, match="refine="):
        plain.refined_relative_poses()
    on = StreamingOdometry(None, streams=2, refine=dict(map_size=2, iters=3))
    assert on._refine_cfg == dict(map_size=2, iters=3) and on.refined_relative_poses().shape == (0, 2, 4, 4)
    src = lambda: "batch"
    assert plain._tap(src) is src and on._tap(src)() == "batch" and on._tapped == "batch"
    od = PWCLONetOdometry(dict(num_input_channels=3, sequence_len=2, num_points=64), device="cpu", refine=dict(map_size=2))
    assert od.refine and od.stream._refine_cfg == dict(map_size=2)


# ---- declarations ----------------------------------------------------------------------------------------------------------

NEW = [("icp_normals_kernel_wrapper", 7), ("icp_queries_kernel_wrapper", 7), ("icp_accumulate_kernel_wrapper", 15),
       ("icp_solve_kernel_wrapper", 14), ("icp_map_push_kernel_wrapper", 14)]


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


def test_every_declared_name_is_exported_and_the_version_stays():
    with open(os.path.join(ROOT, "include", "pwclo_ops.h")) as f:
        header = f.read()
    lib = _lib.load()
    names = set(re.findall(r"\b(icp_\w+)\s*\(", header))
    assert names == {n for n, _ in NEW} | {"icp_accumulate_groups"}
    for n in names:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert lib.pwclo_abi_version() == 1                                          # additions only
    for n in (1, 255, 256, 257, 8192):
        assert lib.icp_accumulate_groups(n) == registration.groups(n) == -(-n // 256)
    assert (registration.ROW, registration.H0, registration.G0, registration.SW, registration.COST, registration.PAIRS) == \
        (model.ROW, model.H0, model.G0, model.SW, model.COST, model.PAIRS)
    with open(os.path.join(ROOT, "pwclonet_pylidarslam_amd", "csrc", "icp.hpp")) as f:
        hpp = f.read()
    assert "ICP_RANK_EPS = 1e-10" in hpp and "ICP_H = 0, ICP_G = 21, ICP_SW = 27, ICP_COST = 28, ICP_PAIRS = 29" in hpp
