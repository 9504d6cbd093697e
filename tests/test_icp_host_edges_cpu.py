"""The arithmetic of csrc/icp.hpp on the host, under AddressSanitizer and UndefinedBehaviorSanitizer: builds
tests/fixtures/icp_host_edges.hip (a stand-alone program, nothing of it is loaded into Python), runs it once and compares
every printed value with tests/icp_model.py, to the bounds of tests/test_gpu_icp_edges.py: eigenvalues within 64 eps64 of
the largest, directions within 64 eps64 / gap, sums within 1e-12 of the sum of the terms' magnitudes, steps and poses
1e-10 norm-wise relative."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import icp_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
S3 = float(np.float32(0.3))
f32 = lambda v: float(np.float32(v))

MATS = [[3.0, 0.0, 0.0, 1.0, 0.0, 2.0], [0.0] * 6, [2.0, 0.0, 0.0, 2.0, 0.0, 5.0], [3.0, 1.0, 1.0, 3.0, 1.0, 3.0],
        [1.0, NAN, 0.0, 2.0, 0.0, 3.0], [NAN, 0.5, 0.0, 2.0, 0.0, 3.0], [1e30, 2e29, -3e29, 4e30, 5e29, 9e30],
        [84.0, -42.0, 0.0, 84.0, 0.0, 0.0], [4.0, 1.0, -2.0, 3.0, 0.5, 6.0], [1.0, 1e-9, 0.0, 1e-18, 0.0, 0.0]]
YS = [[1.0, 2.0, 8.0], [0.0, 0.0, 0.0], [-1.0, -2.0, -8.0]]
HUBER = [(S3, S3), (-S3, S3), (0.0, 0.5), (-0.0, 0.5), (0.25, 0.5), (0.75, 0.5), (f32(6e-5), 5e-5), (f32(1e-4), 5e-5),
         (f32(2e-4), 5e-5), (-f32(6e-5), 5e-5), (f32(4e-5), 5e-5), (1e-4, 5e-5), (NAN, 0.5), (INF, 0.5), (5e-5, 5e-5)]
PAIRS = [(S3, S3), (-S3, S3), (0.0, 0.5), (f32(6e-5), 5e-5), (f32(1e-4), 5e-5), (f32(2e-4), 5e-5), (0.25, 0.5), (3.0, 0.5)]
T = model.pose(np.array([[0.9987502603949663, -0.04997916927067833, 0.0], [0.04997916927067833, 0.9987502603949663, 0.0],
                         [0.0, 0.0, 1.0]]), [0.1, -0.2, 0.05])
RM = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
P, Y = np.array([[1.5, -2.25, 0.75]], dtype=np.float32), np.array([[1.0, 2.0, 0.0]], dtype=np.float32)
N2 = np.array([[0.36, -0.48, 0.8]], dtype=np.float32)
DAMPINGS = (0.0, 1e-6)


def _full(m):
    return np.array([[m[0], m[1], m[2]], [m[1], m[3], m[4]], [m[2], m[4], m[5]]])


def _rows():
    rows = np.zeros((8, model.ROW))
    step345 = np.array([0.0, 0.0, 0.0, 3.0 / 1024, 4.0 / 1024, 0.0])
    th = 3.141592653589793 - 5e-7
    nearpi = np.array([th / 3.0, 2.0 * th / 3.0, 2.0 * th / 3.0, 0.1, -0.2, 0.3])
    for i in range(8):
        for e, (a, b) in enumerate(model.UPPER):
            rows[i, model.H0 + e] = 4.0 if a == b else 0.0
        rows[i, model.SW], rows[i, model.PAIRS] = 1.0, 400.0
    a = np.arange(6)
    rows[0, model.G0:model.G0 + 6], rows[1, model.G0:model.G0 + 6] = -4.0 * step345, -4.0 * nearpi
    for i in (3, 4, 5):
        rows[i, model.G0:model.G0 + 6] = 0.5 * (a + 1)
    rows[7, model.G0:model.G0 + 6] = 0.25 * (a - 2)
    rows[3, model.H0 + 7], rows[4, model.G0 + 2], rows[5, model.SW] = NAN, NAN, NAN
    rows[6, :30] = 0.0
    rows[6, model.H0 + 20], rows[6, model.G0 + 5], rows[6, model.SW], rows[6, model.COST], rows[6, model.PAIRS] = 1.0, 0.25, 1.0, 0.0625, 1.0
    rows[7, model.H0 + 1], rows[7, model.H0 + 9] = 1.0, -0.5
    return rows, step345, nearpi


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc is missing: the host program cannot be built")
    exe = str(tmp_path_factory.mktemp("icp_host_edges") / "icp_host_edges")
    cmd = [hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Xarch_host",
           "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "pwclonet_pylidarslam_amd", "csrc"),
           os.path.join(ROOT, "tests", "fixtures", "icp_host_edges.hip"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-4000:]
    # the caller's environment as it is, with the two option strings added: the sanitizer runtimes are linked into the
    # executable, so nothing is preloaded for them
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert ran.returncode == 0, (ran.returncode, ran.stderr[-4000:])
    assert ran.stderr.strip() == "", ran.stderr[-4000:]                          # the sanitizers reported nothing
    out = {}
    for line in ran.stdout.splitlines():
        label, i, *words = line.split()
        kind = np.uint32 if len(words[0]) == 8 else np.uint64
        out[(label, int(i))] = np.array([int(w, 16) for w in words], dtype=kind).view(np.float32 if kind is np.uint32 else np.float64)
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def test_the_program_ran_on_the_tables_of_this_file(printed):
    """The inputs the program printed are this file's tables, bit for bit (NaNs included)."""
    same = lambda key, want, kind=np.float64: np.array_equal(_bits(printed[key]), _bits(np.array(want, dtype=kind).reshape(-1)))
    for i, m in enumerate(MATS):
        assert same(("in_mat", i), m), i
    for k, y in enumerate(YS):
        assert same(("in_y", k), y, np.float32), k
    for i, h in enumerate(HUBER):
        assert same(("in_huber", i), h), i
    for i, (r, sigma) in enumerate(PAIRS):
        assert same(("in_pair", i), (r, sigma)) and same(("in_q", i), (1.0, 2.0, r), np.float32), i
        assert same(("in_q2", i), (1.25, 1.5, r), np.float32), i
    assert same(("in_T", 0), T[:3]) and same(("in_Rm", 0), RM) and same(("in_p", 0), P, np.float32)
    assert same(("in_map", 0), Y, np.float32) and same(("in_n", 0), (0.0, 0.0, 1.0), np.float32)
    assert same(("in_n", 1), N2, np.float32) and same(("in_damping", 0), DAMPINGS)
    rows = _rows()[0]
    for i in range(8):
        assert same(("in_row", i), rows[i]), i
    assert sum(1 for key in printed if key[0].startswith("in_")) == len(MATS) + 3 + len(HUBER) + 3 * len(PAIRS) + 6 + 1 + 8


def test_eig3_and_normal(printed):
    for i, m in enumerate(MATS):
        val, vec = printed[("eig_val", i)], printed[("eig_vec", i)]
        want_val, want_vec = model.eig3(m)
        finite = np.isfinite(np.array(m)).all()
        assert np.array_equal(np.isnan(val), np.isnan(want_val)) and np.array_equal(np.isnan(vec), np.isnan(want_vec)), i
        if finite:
            w, v = np.linalg.eigh(_full(m))
            scale = max(abs(w).max(), 1e-300)
            assert np.abs(val - w).max() <= 64.0 * model.EPS64 * scale and np.abs(val - want_val).max() <= 64.0 * model.EPS64 * scale, i
            assert (np.diff(val) >= 0.0).all() and abs(np.linalg.norm(vec) - 1.0) <= 4.0 * model.EPS64, i
            gap = (w[1] - w[0]) / scale
            if gap > 1e-6:                                                       # a simple smallest eigenvalue: its direction
                assert 1.0 - abs(vec @ v[:, 0]) <= 64.0 * model.EPS64 / gap, i
            else:                                                                # a repeated one: anywhere in its eigenspace
                assert abs(vec @ v[:, 2]) <= 64.0 * model.EPS64 or w[2] == w[0], i
            assert np.abs(vec - want_vec).max() <= 64.0 * model.EPS64, i         # and the restated solver's own choice
        for k, y in enumerate(YS):
            got = printed[("normal", 3 * i + k)]
            if not want_val[1] > model.RANK_EPS * want_val[2]:                   # NaN fails the rank test
                assert not got.view(np.uint32).any(), (i, k)
                continue
            d = float(want_vec @ np.array(y))
            want = (-1.0 if d > 0.0 else 1.0) * want_vec
            assert np.abs(got - want.astype(np.float32)).max() <= 2.0 ** -23, (i, k)
            assert float(got.astype(np.float64) @ np.array(y)) <= 0.0 or abs(d) <= 64.0 * model.EPS64 * 8.5, (i, k)
    zero = [i for i, m in enumerate(MATS) if not printed[("normal", 3 * i)].any()]
    # the zero matrix, a NaN on the diagonal, rank one; not the planar one.  Not matrix 4 either: the sweeps skip a NaN off
    # the diagonal as they skip a zero, so the diagonal (1, 2, 3) decides alone.  A NaN or Inf point gives a covariance whose
    # diagonal is not finite as well, and that fails the rank test (matrix 5).
    assert zero == [1, 5, 9] and printed[("eig_val", 4)].tolist() == [1.0, 2.0, 3.0]
    assert printed[("normal", 3 * 7 + 1)].tolist() == [0.0, 0.0, 1.0]            # planar in z = 0, y at the origin: no flip
    assert printed[("eig_vec", 0)].tolist() == [0.0, 1.0, 0.0] and printed[("eig_val", 0)].tolist() == [1.0, 2.0, 3.0]
    assert printed[("eig_vec", 2)].tolist() == [1.0, 0.0, 0.0]                   # equal eigenvalues: the lower index


def test_huber_and_add_pair(printed):
    for i, (r, sigma) in enumerate(HUBER):
        got = printed[("huber", i)][0]
        with np.errstate(invalid="ignore"):
            want = float(model.huber_w2(np.float64(r), sigma))
        assert (np.isnan(got) and np.isnan(want)) or abs(got - want) <= 4.0 * model.EPS64 * abs(want), (i, got, want)
        assert np.isnan(want) or (np.isfinite(got) and got > 0.0), i
    assert printed[("huber", 2)][0] == printed[("huber", 3)][0] == printed[("huber", 4)][0] == 1.0
    assert printed[("huber", 14)][0] == (2.0 * 5e-5 * 5e-5 - 5e-5 * 5e-5) / (1e-4 * 1e-4)    # |r| == sigma below the clamp
    one = lambda a: np.asarray(a)[None]
    live = np.ones((1,), dtype=np.int32)
    total, total_mag = np.zeros((model.ROW,)), np.zeros((model.ROW,))
    for i, (r, sigma) in enumerate(PAIRS):
        q = np.array([[1.0, 2.0, r]], dtype=np.float32)
        want, mag = model.accumulate(P, one(q), np.zeros((1, 1), dtype=np.int32), np.zeros((1, 1), dtype=np.float32), one(Y),
                                     one(np.array([[0.0, 0.0, 1.0]], dtype=np.float32)), live, one(RM), T, sigma, 1.0)
        got = printed[("pair", i)]
        assert got.shape == (30,) and (np.abs(got - want[:30]) <= 1e-12 * mag[:30]).all() and got[model.PAIRS] == 1.0, i
        q2 = np.array([[1.25, 1.5, r]], dtype=np.float32)
        w2, m2 = model.accumulate(P, one(q2), np.zeros((1, 1), dtype=np.int32), np.zeros((1, 1), dtype=np.float32), one(Y),
                                  one(N2), live, one(RM), T, 0.5, 1.0)
        total, total_mag = total + w2, total_mag + m2
    got = printed[("pair_sum", 0)]
    assert (np.abs(got - total[:30]) <= 1e-12 * total_mag[:30]).all() and got[model.PAIRS] == len(PAIRS)


def test_solve6_and_update_pose(printed):
    rows, step345, nearpi = _rows()
    refused = []
    for i in range(8):
        for d, damping in enumerate(DAMPINGS):
            key = 2 * i + d
            ok, delta = printed[("solve_ok", key)][0], printed[("solve", key)]
            want = model.solve(rows[i], T, 0, 0, damping, 0.0, 1)
            assert (ok == 0.0) == (want["status"] == model.BAD_PIVOT), (i, d)
            if ok == 0.0:
                refused.append(key)
                assert delta.tolist() == [7.0] * 6 and ("update", key) not in printed, (i, d)     # delta untouched
                continue
            scale = np.abs(want["delta"]).max()
            assert np.abs(delta - want["delta"]).max() <= 1e-10 * scale, (i, d)
            got = printed[("update", key)].reshape(3, 4)
            new = model.exp_update(delta, T)
            assert np.abs(got - new[:3]).max() <= 1e-10 * np.abs(new[:3]).max(), (i, d)
            assert np.abs(got[:, :3] @ got[:, :3].T - np.eye(3)).max() <= 1e-14, (i, d)
    assert refused == [6, 7, 8, 9, 10, 11, 12]           # a NaN in H, in g, in sw under either damping; the one pair under 0
    assert np.array_equal(printed[("solve", 0)], step345) and np.linalg.norm(printed[("solve", 0)]) == 5.0 / 1024
    assert np.array_equal(printed[("solve", 2)], nearpi) and abs(np.linalg.norm(nearpi[:3]) - np.pi) < 1e-6
    assert not printed[("solve", 4)].any()                                       # g = 0: a zero step
    zero = printed[("update_zero", 0)].reshape(3, 4)
    assert np.abs(zero - T[:3]).max() <= 1e-15 and np.array_equal(zero, printed[("update", 4)].reshape(3, 4))
