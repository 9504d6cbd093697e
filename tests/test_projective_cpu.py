"""CPU checks of the projective registration: the NumPy model of tests/projective_model.py against
fixtures recorded by running the reference (tools/gen_projective_golden.py -> tests/golden/projective_cases.npz), the
model's tie rule, the documented departure from the reference, the new ABI surface and the ``refine=dict(kind=...)`` rules."""
import ctypes
import os
import re

import numpy as np
import pytest

import projective_model as model
from pwclonet_pylidarslam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "projective_cases.npz")


def load_cases():
    z = np.load(GOLDEN)
    out = []
    for i in range(int(z["cases"])):
        c = {k[len("c%d_" % i):]: z[k] for k in z.files if k.startswith("c%d_" % i)}
        H, W, up, down = c["image"]
        c["im"] = model.image(int(H), int(W), float(up), float(down))
        out.append(c)
    return out


CASES = load_cases()
IDS = ["%dx%d_fov%g" % (c["im"]["H"], c["im"]["W"], c["image"][2]) for c in CASES]


def test_fixture_shapes_cover_the_issue():
    assert {(c["im"]["H"], c["im"]["W"]) for c in CASES} == {(16, 64), (5, 60), (8, 33)}
    assert {(c["image"][2], c["image"][3]) for c in CASES} == {(3.0, -24.8), (15.0, -15.0)}
    for c in CASES:
        pts, lengths = c["points"], c["lengths"]
        assert 600 <= pts.shape[1] <= 2000 and (lengths < pts.shape[1]).any()
        assert not pts[-1].any()                                                    # one empty cloud
        for cloud in pts[:-1]:
            assert ((cloud == 0).all(axis=1)).any()                                 # points at the origin
            assert ((cloud[:, 1] == 0) & np.signbit(cloud[:, 1]) & (cloud[:, 0] < 0)).any()      # y = -0.0, x < 0
            uniq = np.unique(cloud[(cloud != 0).any(axis=1)], axis=0, return_counts=True)[1]
            assert (uniq > 1).any()                                                 # identical coordinates


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_pixels_winners_and_vertex_maps_equal_the_reference(c):
    im = c["im"]
    H, W = im["H"], im["W"]
    for k, cloud in enumerate(c["points"]):
        row, col, r, valid, margin = model.pixels(cloud, im)
        ref_valid = (c["ref_row"][k] >= 0) & (c["ref_row"][k] <= H - 1) & (c["ref_col"][k] >= 0) & (c["ref_col"][k] <= W - 1)
        assert np.array_equal(valid, ref_valid)
        assert np.array_equal(row[valid], c["ref_row"][k][valid]) and np.array_equal(col[valid], c["ref_col"][k][valid])
        assert (margin[np.isfinite(margin)] >= 1e-3).all()
        low = (cloud[:, 1] == 0) & np.signbit(cloud[:, 1]) & (cloud[:, 0] < 0)
        assert (c["ref_col"][k][low] == W).all() and not valid[low].any()           # column W: invalid
        vmap, rows = model.vertex_map(cloud, im, c["lengths"][k])
        assert vmap.tobytes() == c["ref_vmap"][k].tobytes()                          # bit-equal
        # several points share a pixel, the nearest stands; equal points: the lowest row
        offered = valid & (np.arange(len(cloud)) < c["lengths"][k])
        pix = row * W + col
        if offered.any():
            counts = np.bincount(pix[offered], minlength=H * W)
            assert k == len(c["points"]) - 1 or (counts > 1).any()
        win = rows.reshape(-1)
        for p in np.flatnonzero(win >= 0)[::7]:
            same = np.flatnonzero(offered & (pix == p))
            best = same[np.lexsort((same, r[same]))][0]
            assert win[p] == best
    assert (model.vertex_map(c["points"][-1], im, c["lengths"][-1])[1] == -1).all()  # the empty cloud


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_normals_against_the_reference(c, capsys):
    """The zero / non-zero pattern is the reference's; the direction error 1 - |n . n_ref| of the fp64 model against the
    reference's fp32 normals is the reference's own fp32 error: measured and printed, the yardstick of the GPU test."""
    worst = 0.0
    for k in (3, 5):
        for i, vmap in enumerate(c["ref_vmap"]):
            n, det = model.normal_map(vmap, k)
            ref = c["ref_nmap%d" % k][i].astype(np.float64)
            assert np.array_equal((n != 0).any(axis=-1), (ref != 0).any(axis=-1))
            occupied = (vmap != 0).any(axis=-1)
            assert not ((np.abs(det[occupied]) > 1e-6 / 4) & (np.abs(det[occupied]) < 4e-6)).any()
            nz = (n != 0).any(axis=-1)
            if nz.any():
                err = 1.0 - np.abs((n[nz] * ref[nz]).sum(axis=-1))
                worst = max(worst, float(err.max()))
                assert ((n[nz] * vmap[nz]).sum(axis=-1) > 0).all()                   # away from the sensor
    with capsys.disabled():
        print("\n[projective] %s: reference fp32 normal direction error vs fp64, max = %.3e" % (
            "%dx%d" % (c["im"]["H"], c["im"]["W"]), worst))
    assert worst < 0.5


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_neighbours_and_slots_equal_the_reference(c):
    im = c["im"]
    H, W = im["H"], im["W"]
    target, stack, normals = c["ref_vmap"][0], c["ref_vmap"][1:3], c["ref_nmap5"][1:3]
    a = model.associate(target, stack, np.ones_like(stack), np.eye(4), im, np.inf)
    occupied = (target != 0).any(axis=-1).reshape(-1)
    assert np.array_equal(a["pixel"][occupied], np.flatnonzero(occupied))            # T = I: a point's pixel is its own
    paired = a["slot"] >= 0
    assert (a["gap"][paired] >= 1e-4).all()
    mine_v, mine_n = np.zeros((H * W, 3), dtype=np.float32), np.zeros((H * W, 3), dtype=np.float32)
    at = np.flatnonzero(paired)
    mine_v[at] = stack.reshape(2, H * W, 3)[a["slot"][at], at]
    mine_n[at] = normals.reshape(2, H * W, 3)[a["slot"][at], at]
    assert mine_v.tobytes() == c["ref_neighbor_v"].reshape(H * W, 3).tobytes()
    ref_n = c["ref_neighbor_n"].reshape(H * W, 3)
    assert mine_n[at].tobytes() == ref_n[at].tobytes()
    assert paired.sum() > H * W // 4


def test_tie_rule_lowest_row_and_lower_slot():
    im = model.image(8, 33, 3.0, -24.8)
    d = model.beams(im)[[40, 40, 40, 100]]
    pts = (d * np.array([[5.0], [5.0], [4.0], [3.0]])).astype(np.float32)
    pts[1] = pts[0]
    _, rows = model.vertex_map(pts[[0, 1]], im, 2)
    assert rows.reshape(-1)[40] == 0                                                 # identical points: the lowest row
    _, rows = model.vertex_map(pts, im, 4)
    assert rows.reshape(-1)[40] == 2 and rows.reshape(-1)[100] == 3                  # the nearest range wins
    _, rows = model.vertex_map(pts, im, 2, keep=np.array([0, 1, 1, 1]))
    assert rows.reshape(-1)[40] == 1 and rows.reshape(-1)[100] == -1                 # lengths and keep both bind
    vmap = np.zeros((8, 33, 3), dtype=np.float32)
    vmap.reshape(-1, 3)[40] = pts[0]
    y = np.zeros((3, 8, 33, 3), dtype=np.float32)
    y.reshape(3, -1, 3)[1:, 40] = pts[0] * np.float32(1.01)                          # slots 1 and 2 hold the same point
    a = model.associate(vmap, y, np.ones_like(y), np.eye(4), im, 1.0)
    assert a["slot"][40] == 1 and a["gap"][40] == 0.0


def test_departure_every_source_point_pairs_on_its_own():
    """Two source points that land on one pixel: two pairs here, one in the reference, which z-buffers the moved points
    among themselves first (nearest_neighbor_search's new_target_vmap; restated with the model's vertex_map)."""
    im = model.image(8, 33, 3.0, -24.8)
    H, W = 8, 33
    jitter = np.zeros((H * W, 2))
    a, b = 3 * W + 10, 3 * W + 11
    jitter[a, 1], jitter[b, 1] = 0.4, -0.4                                           # columns 10.4 and 10.6
    d = model.beams(im, jitter)
    vmap = np.zeros((H * W, 3), dtype=np.float32)
    vmap[a], vmap[b] = d[a] * 5.0, d[b] * 6.0
    assert model.vertex_map(vmap, im, H * W)[1].reshape(-1)[[a, b]].tolist() == [a, b]
    yaw = -0.3 * 2.0 * np.pi / W                                                     # + 0.3 columns: 10.7 and 10.9 -> 11
    T = np.eye(4)
    T[:3, :3] = model.icp.rot([0.0, 0.0, 1.0], yaw)
    target = np.zeros((1, H * W, 3), dtype=np.float32)
    target[0, b] = d[b] * 5.5
    normals = np.zeros_like(target)
    normals[0, b] = d[b]
    row, _, assoc = model.accumulate(vmap.reshape(H, W, 3), target.reshape(1, H, W, 3), normals.reshape(1, H, W, 3), T, im,
                                     0.5, 1.0)
    assert assoc["pixel"][[a, b]].tolist() == [b, b] and row[model.icp.PAIRS] == 2.0
    moved = assoc["q32"]
    ref_target = model.vertex_map(moved, im, H * W)[0].reshape(-1, 3)
    assert ((ref_target != 0).any(axis=1)).sum() == 1                                # the reference keeps the nearer one


NEW = [("proj_vertex_map_kernel_wrapper", 13), ("proj_normal_map_kernel_wrapper", 6), ("proj_model_build_kernel_wrapper", 14),
       ("proj_accumulate_kernel_wrapper", 15), ("proj_map_push_kernel_wrapper", 12)]


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
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    lib = _lib.load()
    names = set(re.findall(r"\b(proj_\w+)\s*\(", header))
    assert names == {n for n, _ in NEW} | {"proj_vertex_map_workspace_bytes", "proj_model_build_workspace_bytes"}
    for n in names:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert lib.pwclo_abi_version() == 1                                              # additions only
    assert lib.proj_vertex_map_workspace_bytes(2, 16, 64) == 2 * 16 * 64 * 8
    assert lib.proj_model_build_workspace_bytes(2, 3, 16, 64) == 2 * 3 * 16 * 64 * 8
    assert lib.proj_vertex_map_workspace_bytes(0, 16, 64) == 0 and lib.proj_model_build_workspace_bytes(1, 0, 1, 1) == 0


def test_refine_kind_argument_rules():
    from pwclonet_pylidarslam_amd import projective
    from pwclonet_pylidarslam_amd.odometry import StreamingOdometry
    sweeps = dict(dataset="kitti360", capacity=4096)
    with pytest.raises(ValueError, match="sweeps"):
        StreamingOdometry(None, streams=2, refine=dict(kind="projective", height=8, width=64))
    with pytest.raises(ValueError, match="per_stream"):
        StreamingOdometry(None, streams=2, sweeps=sweeps, per_stream=True,
                          refine=dict(kind="projective", height=8, width=64, per_stream=True))
    with pytest.raises(ValueError, match="kind"):
        StreamingOdometry(None, streams=2, sweeps=sweeps, refine=dict(kind="voxel"))
    with pytest.raises(ValueError, match="voxel_size"):
        StreamingOdometry(None, streams=2, sweeps=dict(sweeps, voxel_size=0.3), refine=dict(kind="projective"))
    assert StreamingOdometry(None, streams=2, sweeps=sweeps, refine=dict(kind="projective"))._refine_kind == "projective"
    assert StreamingOdometry(None, streams=2, refine=dict(kind="knn", map_size=2))._refine_cfg == dict(map_size=2)
    assert StreamingOdometry(None, streams=2, refine=dict(map_size=2))._refine_kind == "knn"
    with pytest.raises(ValueError, match="lock step only"):
        projective.ProjectiveIcpRefiner(2, 1024, per_stream=True)
    with pytest.raises(ValueError, match="kernel_size"):
        projective.ProjectiveIcpRefiner(2, 1024, kernel_size=7)
