"""GPU parity tests of the HIP operator stack against the CPU oracle (run with ``-m gpu``).

Every call goes through the C ABI of libpwclo_hip.so (``pointnet2_ops._ext`` is a thin ctypes
front-end).  Bars: bit-exact for every index output (FPS, knn, ball_query, three_nn) and for
the copy / interpolation outputs whose operation order is fixed; 1e-5 relative for the atomic
scatter-add gradients (order-dependent fp32 sums; oracle accumulates in double).
"""
import numpy as np
import pytest
import torch

from oracle import ops as O
from pwclonet_pylidarslam_amd.pointnet2_ops import _ext as E
from pwclonet_pylidarslam_amd import synthetic

pytestmark = pytest.mark.gpu


def g(t, dev):
    return t.to(dev)


def rand_cloud(seed, b, n, scale=20.0):
    gen = torch.Generator().manual_seed(seed)
    return (torch.rand(b, n, 3, generator=gen) * 2 - 1) * scale


# ---------------------------------------------------------------- furthest point sampling
FPS_SHAPES = [(2, 8192, 2048), (2, 2048, 1024), (3, 1024, 256), (3, 256, 64), (2, 1024, 2048),
              (2, 100, 50), (2, 63, 20), (1, 5000, 300), (2, 16384, 128), (1, 20000, 64),
              (1, 30000, 12), (2, 1, 3), (2, 129, 129), (2, 511, 40), (2, 4096, 512), (1, 4097, 300),
              # the dispatch rows no other shape reaches (n = 128: one wave, two residues per thread; n = 512 on a random
              # cloud), the last n with the LDS point table and the first without it, the largest single-workgroup
              # cloud (48 points per thread exactly) and the first cooperative one (two workgroups)
              (2, 128, 40), (2, 512, 40), (1, 10236, 24), (1, 10237, 24), (1, 24576, 16), (1, 24577, 16)]


@pytest.mark.parametrize("b,n,m", FPS_SHAPES)
def test_fps_random(cuda, b, n, m):
    x = rand_cloud(100 + n + m, b, n)
    ref = O.furthest_point_sampling(x, m)
    out = E.furthest_point_sampling(g(x, cuda), m).cpu()
    assert torch.equal(out, ref)


@pytest.mark.parametrize("n,m", [(512, 300), (1000, 700), (8192, 512), (64, 64), (300, 200), (8192, 2048)])
def test_fps_exact_ties_lattice(cuda, n, m):
    """Integer lattice + duplicates: almost every arg-max is an exact tie, so the result is
    decided by the reference's tie rule (bit-reversed k mod bs, then k div bs)."""
    gen = torch.Generator().manual_seed(n * 7 + m)
    x = torch.randint(-3, 4, (3, n, 3), generator=gen).float()
    ref = O.furthest_point_sampling(x, m)
    out = E.furthest_point_sampling(g(x, cuda), m).cpu()
    assert torch.equal(out, ref)


def test_fps_origin_points_and_exhaustion(cuda):
    """Zero padding is never sampled (|p|^2 <= 1e-3), index 0 is always first even when it is
    padding, and once the valid points run out the reference keeps returning duplicates."""
    gen = torch.Generator().manual_seed(5)
    x = (torch.rand(3, 700, 3, generator=gen) * 2 - 1) * 10
    x[0, :350] = 0.0                      # first half padding, incl. index 0
    x[1, 100:] = 0.01                     # |p|^2 = 3e-4 <= 1e-3: skipped
    x[2] = 0.0                            # nothing valid at all -> all zeros
    m = 400
    ref = O.furthest_point_sampling(x, m)
    out = E.furthest_point_sampling(g(x, cuda), m).cpu()
    assert torch.equal(out, ref)
    assert (out[2] == 0).all()
    assert (out[0, 1:] >= 350).all()   # padding (indices < 350) is never sampled after index 0


def test_fps_kitti_shaped_batch32(cuda):
    """Full benchmark size (B=32, N=8192 -> 2048): oracle parity on 2 clouds, plus
    size-independent properties on all 32: first index 0, no repeated index."""
    pc1, _, _, _ = synthetic.kitti_like_pair(77, 8192, 4)
    x = torch.from_numpy(np.tile(pc1[:, :, :3], (8, 1, 1))).contiguous()
    x = x + torch.arange(32).reshape(32, 1, 1) * 1e-3  # make the 32 clouds distinct
    out = E.furthest_point_sampling(g(x, cuda), 2048).cpu()
    assert (out[:, 0] == 0).all()
    for b in range(32):
        assert len(torch.unique(out[b])) == 2048
    ref = O.furthest_point_sampling(x[:2].contiguous(), 2048)
    assert torch.equal(out[:2], ref)


def test_fps_batch16_ties_and_padding(cuda):
    """A 16-cloud batch of lattice clouds (almost every arg-max is a tie) with zero padding in some
    of them: every cloud independently follows the reference's tie rule."""
    gen = torch.Generator().manual_seed(2024)
    x = torch.randint(-6, 7, (16, 5000, 3), generator=gen).float()
    x[3, :1000] = 0.0
    x[8, 2500:] = 0.0
    ref = O.furthest_point_sampling(x, 300)
    out = E.furthest_point_sampling(g(x, cuda), 300).cpu()
    assert torch.equal(out, ref)


def test_fps_large_cloud_spatial_orders_agree(cuda, monkeypatch):
    """The large-cloud sampler's spatial order comes from hand-written kernels (csrc/sampling.hip fps_spatial_order: counting
    sort into aspect-aware Morton cells + a priority sort per 1024 positions) or, as the A/B reference, from torch sorts:
    any such order is exact, so both give the oracle's indices -- also with zero padding and on a tie lattice."""
    from pwclonet_pylidarslam_amd.pointnet2_ops import _ext as ext
    gen = torch.Generator().manual_seed(77)
    x = (torch.rand(2, 40000, 3, generator=gen) * 2 - 1) * torch.tensor([60.0, 60.0, 2.0])
    x[0, 30000:] = 0.0
    x[1] = torch.randint(-12, 13, (40000, 3), generator=gen).float()
    ref = O.furthest_point_sampling(x, 96)
    for order in ("device", "torch"):
        monkeypatch.setattr(ext, "LARGE_CLOUD_ORDER", order)
        assert torch.equal(ext.furthest_point_sampling(g(x, cuda), 96).cpu(), ref), order


@pytest.mark.parametrize("b,n,m,lattice", [(3, 30000, 150, 0), (2, 40001, 120, 9), (9, 25000, 40, 0),
                                           # BASELINE configs[4] at its real size (G = 8 workgroups per cloud, 8191
                                           # alternations of the two exchange slot sets): random, a lattice with
                                           # exact ties at every decision, and a lattice with fewer distinct points
                                           # than samples (19^3 = 6859 < 8192: exhaustion, distance-0 ties)
                                           (1, 120000, 8192, 0), (1, 120000, 8192, 30), (1, 120000, 8192, 9)])
def test_fps_large_cloud_cooperative(cuda, b, n, m, lattice):
    """n > 24576: several workgroups share a cloud and exchange their arg-max through global memory
    (csrc/sampling.hip: fps_coop_kernel); same indices as the oracle, ties and zero padding included."""
    gen = torch.Generator().manual_seed(n + m)
    if lattice:
        x = torch.randint(-lattice, lattice + 1, (b, n, 3), generator=gen).float()
    else:
        x = (torch.rand(b, n, 3, generator=gen) * 2 - 1) * 40
    x[0, 100:5000] = 0.0
    ref = O.furthest_point_sampling(x, m)
    out = E.furthest_point_sampling(g(x, cuda), m).cpu()
    assert torch.equal(out, ref)


def test_fps_cooperative_timeout_is_reported(cuda, monkeypatch):
    """The cooperative sampler must never continue silently (reference contract: cuda_utils.h:30-39 exits).
    PWCLO_FPS_COOP_DEBUG_TIMEOUT=1 shrinks the spin bound and makes the last workgroup of each cloud leave at
    once -- what a non-resident peer looks like; the others give up, the kernel posts PWCLO_ECOOP_TIMEOUT into
    the library's pinned error word and the host raises at the next check.  Run once."""
    from pwclonet_pylidarslam_amd import _lib
    gen = torch.Generator().manual_seed(5)
    x = (torch.rand(1, 40000, 3, generator=gen) * 2 - 1) * 40
    xg = g(x, cuda)
    monkeypatch.setenv("PWCLO_FPS_COOP_DEBUG_TIMEOUT", "1")
    E.furthest_point_sampling(xg, 64)                       # the launch itself succeeds (asynchronous)
    monkeypatch.delenv("PWCLO_FPS_COOP_DEBUG_TIMEOUT")
    with pytest.raises(RuntimeError, match="co-resident"):
        _lib.synchronize(cuda)
    torch.cuda.synchronize()
    _lib.synchronize(cuda)                                   # reported once, then clear
    out = E.furthest_point_sampling(xg, 64).cpu()            # and the library keeps working
    assert torch.equal(out, O.furthest_point_sampling(x, 64))
    # the same failure also surfaces at the next library CALL made after the kernel ran
    monkeypatch.setenv("PWCLO_FPS_COOP_DEBUG_TIMEOUT", "1")
    E.furthest_point_sampling(xg, 64)
    monkeypatch.delenv("PWCLO_FPS_COOP_DEBUG_TIMEOUT")
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="co-resident"):
        E.gather_points(g(torch.zeros(1, 3, 8), cuda), g(torch.zeros(1, 4, dtype=torch.int32), cuda))


def test_fps_two_large_cloud_batches_in_flight_with_the_plain_launch(cuda):
    """bench.py --config 5 keeps TWO batches in flight: the cooperative-launch API would run their samplers one after
    the other (one cooperative queue per device), so that mode selects the plain launch
    (pwclo_fps_large_cloud_launch(0)).  Two such samplers on two streams, 2 x 8 clouds x 8 workgroups side by side,
    return exactly what one cooperative launch returns for each batch (which test_fps_large_cloud_cooperative pins to
    the C oracle), and no time-out is reported.  Run once."""
    from pwclonet_pylidarslam_amd import _lib
    gen = torch.Generator().manual_seed(9)
    xa = g((torch.rand(8, 60000, 3, generator=gen) * 2 - 1) * 40, cuda)
    xb = g((torch.rand(8, 60000, 3, generator=gen) * 2 - 1) * 40, cuda)
    ref_a = E.furthest_point_sampling(xa, 700)
    ref_b = E.furthest_point_sampling(xb, 700)
    torch.cuda.synchronize()
    lib = _lib.load()
    lib.pwclo_fps_large_cloud_launch(0)
    try:
        sa, sb = torch.cuda.Stream(device=cuda), torch.cuda.Stream(device=cuda)
        main = torch.cuda.current_stream(cuda)
        sa.wait_stream(main)
        sb.wait_stream(main)
        outs = []
        for rep in range(2):
            with torch.cuda.stream(sa):
                oa = E.furthest_point_sampling(xa, 700)
            with torch.cuda.stream(sb):
                ob = E.furthest_point_sampling(xb, 700)
            outs.append((oa, ob))
        main.wait_stream(sa)
        main.wait_stream(sb)
        _lib.synchronize(cuda)                               # raises if a workgroup timed out waiting for its peers
    finally:
        lib.pwclo_fps_large_cloud_launch(1)
    for oa, ob in outs:
        assert torch.equal(oa, ref_a) and torch.equal(ob, ref_b)


def test_fps_large_cloud_exchange_modes_agree(cuda):
    """The large-cloud sampler posts through the XCD's L2 when a launch finds all workgroups of a cloud on one XCD
    (checked inside every launch) and with agent-scope stores otherwise; pwclo_fps_large_cloud_exchange(0) forces the
    second protocol.  Both return the same indices (the default mode is pinned to the C oracle by
    test_fps_large_cloud_cooperative).  Run once."""
    from pwclonet_pylidarslam_amd import _lib
    gen = torch.Generator().manual_seed(21)
    x = g((torch.rand(3, 70001, 3, generator=gen) * 2 - 1) * 40, cuda)
    ref = E.furthest_point_sampling(x, 900)
    lib = _lib.load()
    lib.pwclo_fps_large_cloud_exchange(0)
    try:
        got = E.furthest_point_sampling(x, 900)
        _lib.synchronize(cuda)
    finally:
        lib.pwclo_fps_large_cloud_exchange(1)
    assert torch.equal(got, ref)


# ---------------------------------------------------------------- gather / group (+ grads)
@pytest.mark.parametrize("b,c,n,m", [(2, 3, 8192, 2048), (3, 3, 256, 64), (2, 7, 100, 33), (1, 64, 1024, 1),
                                     (2, 3, 50000, 4096), (30, 16, 512, 128)])
def test_gather_points(cuda, b, c, n, m):
    gen = torch.Generator().manual_seed(b * c + n)
    p = torch.randn(b, c, n, generator=gen)
    idx = torch.randint(0, n, (b, m), generator=gen, dtype=torch.int32)
    assert torch.equal(E.gather_points(g(p, cuda), g(idx, cuda)).cpu(), O.gather_points(p, idx))
    go = torch.randn(b, c, m, generator=gen)
    ref = O.gather_points_grad(go, idx, n)
    out = E.gather_points_grad(g(go, cuda), g(idx, cuda), n).cpu()
    torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-5)


GROUP_SHAPES = [(2, 3, 8192, 2048, 32), (2, 16, 2048, 1024, 32), (2, 64, 256, 64, 16),
                (2, 64, 1024, 2048, 8), (2, 3, 256, 256, 6), (1, 5, 77, 13, 3), (2, 64, 256, 256, 4),
                (1, 129, 50, 7, 5)]


@pytest.mark.parametrize("b,c,n,s,k", GROUP_SHAPES)
def test_group_points(cuda, b, c, n, s, k):
    gen = torch.Generator().manual_seed(c * n + s * k)
    p = torch.randn(b, c, n, generator=gen)
    idx = torch.randint(0, n, (b, s, k), generator=gen, dtype=torch.int32)
    out = E.group_points(g(p, cuda), g(idx, cuda)).cpu()
    assert torch.equal(out, O.group_points(p, idx))


# shapes reach every dispatch of the LDS-accumulating kernel: 8 / 4 / 2 / 1 channels per slice (n up to 32768),
# position ranges split over several workgroups (few clouds x slices) or not (>= 64), odd P (scalar loads), and
# the global-atomic fallback (n > 32768)
@pytest.mark.parametrize("b,c,n,s,k", [(2, 16, 2048, 1024, 32), (2, 64, 256, 64, 16), (1, 5, 77, 13, 3),
                                       (16, 64, 1024, 512, 8), (2, 12, 8192, 1000, 4), (3, 9, 16000, 300, 7),
                                       (2, 5, 30000, 700, 3), (1, 4, 40000, 600, 4), (40, 16, 100, 50, 2)])
def test_group_points_grad(cuda, b, c, n, s, k):
    gen = torch.Generator().manual_seed(c * n + s * k + 1)
    go = torch.randn(b, c, s, k, generator=gen)
    idx = torch.randint(0, n, (b, s, k), generator=gen, dtype=torch.int32)
    out = E.group_points_grad(g(go, cuda), g(idx, cuda), n).cpu()
    torch.testing.assert_close(out, O.group_points_grad(go, idx, n), rtol=1e-5, atol=1e-4)


def test_group_points_linearity_full_size(cuda):
    """B=32 at the largest call of the forward (C=64,N=1024,S=2048,K=8): group(a*x+y) ==
    a*group(x)+group(y) exactly for power-of-two a, and every element equals its source."""
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(32, 64, 1024, generator=gen).to(cuda)
    y = torch.randn(32, 64, 1024, generator=gen).to(cuda)
    idx = torch.randint(0, 1024, (32, 2048, 8), generator=gen, dtype=torch.int32).to(cuda)
    gx, gy = E.group_points(x, idx), E.group_points(y, idx)
    assert torch.equal(E.group_points(2 * x + y, idx), 2 * gx + gy)
    ref = torch.gather(x.unsqueeze(2).expand(-1, -1, 2048, -1), 3,
                       idx.long().unsqueeze(1).expand(-1, 64, -1, -1))
    assert torch.equal(gx, ref)


# ---------------------------------------------------------------- ball query
@pytest.mark.parametrize("b,m,n,k,r", [(2, 2048, 8192, 32, 0.5), (2, 1024, 2048, 32, 1.0),
                                        (2, 256, 1024, 16, 2.0), (2, 64, 256, 16, 4.0),
                                        (1, 33, 100, 5, 1e-6), (1, 33, 100, 7, 1e6)])
def test_ball_query(cuda, b, m, n, k, r):
    xyz = rand_cloud(3 * m + n, b, n, scale=8.0)
    new_xyz = xyz[:, :m].contiguous() + 0.01
    ref = O.ball_query(new_xyz, xyz, r, k)
    out = E.ball_query(g(new_xyz, cuda), g(xyz, cuda), r, k).cpu()
    assert torch.equal(out, ref)


# ---------------------------------------------------------------- three_nn / three_interpolate
@pytest.mark.parametrize("b,n,m", [(2, 256, 64), (2, 1024, 256), (2, 2048, 1024), (1, 10, 2), (1, 10, 1),
                                   (1, 70, 3)])
def test_three_nn(cuda, b, n, m):
    unknown = rand_cloud(n + m, b, n)
    known = rand_cloud(n * m + 1, b, m)
    if m >= 4:
        known[:, 1] = known[:, 0]  # exact duplicate: tie must go to the lower index
    d_ref, i_ref = O.three_nn(unknown, known)
    d, i = E.three_nn(g(unknown, cuda), g(known, cuda))
    assert torch.equal(i.cpu(), i_ref)
    assert torch.equal(d.cpu(), d_ref)


@pytest.mark.parametrize("b,c,m,n", [(2, 64, 64, 256), (2, 64, 256, 1024), (1, 5, 9, 31), (20, 64, 300, 1200),
                                     (1, 6, 20000, 5000), (2, 3, 40000, 900)])
def test_three_interpolate(cuda, b, c, m, n):
    gen = torch.Generator().manual_seed(c + m + n)
    p = torch.randn(b, c, m, generator=gen)
    idx = torch.randint(0, m, (b, n, 3), generator=gen, dtype=torch.int32)
    w = torch.rand(b, n, 3, generator=gen)
    out = E.three_interpolate(g(p, cuda), g(idx, cuda), g(w, cuda)).cpu()
    assert torch.equal(out, O.three_interpolate(p, idx, w))
    go = torch.randn(b, c, n, generator=gen)
    gout = E.three_interpolate_grad(g(go, cuda), g(idx, cuda), g(w, cuda), m).cpu()
    torch.testing.assert_close(gout, O.three_interpolate_grad(go, idx, w, m), rtol=1e-5, atol=1e-4)


# ---------------------------------------------------------------- knn
KNN_SHAPES = [  # (K, N, S) of the 23 calls in one forward, B=2
    (32, 8192, 2048), (32, 2048, 1024), (16, 1024, 256), (16, 256, 64), (32, 256, 256), (4, 256, 256),
    (8, 64, 256), (6, 256, 256), (8, 256, 1024), (6, 1024, 1024), (4, 1024, 1024), (8, 1024, 2048),
    (6, 2048, 2048), (4, 2048, 2048),
    # edge shapes
    (1, 97, 33), (5, 5, 7), (64, 64, 3), (64, 1000, 17), (3, 130, 1), (32, 33, 50)]


@pytest.mark.parametrize("k,n,s", KNN_SHAPES)
def test_knn_random(cuda, k, n, s):
    xyz = rand_cloud(k * 1000 + n + s, 2, n)
    new_xyz = rand_cloud(k * 1000 + n + s + 1, 2, s)
    if s <= n:
        new_xyz[0] = xyz[0, :s]  # self-queries in one cloud: first neighbour is the point itself
    d_ref, i_ref = O.knn_point_with_dist(k, xyz, new_xyz)
    d, i = E.knn_point(k, g(xyz, cuda), g(new_xyz, cuda), return_dist=True)
    assert torch.equal(i.cpu(), i_ref)
    assert torch.equal(d.cpu(), d_ref)   # also proves the device sqrtf is correctly rounded


def test_knn_duplicates_and_lattice(cuda):
    """Exact distance ties (duplicated points, integer lattice): lower index first."""
    gen = torch.Generator().manual_seed(11)
    xyz = torch.randint(-4, 5, (2, 2000, 3), generator=gen).float()
    new_xyz = xyz[:, ::7].contiguous()
    for k in (4, 16, 32):
        d_ref, i_ref = O.knn_point_with_dist(k, xyz, new_xyz)
        d, i = E.knn_point(k, g(xyz, cuda), g(new_xyz, cuda), return_dist=True)
        assert torch.equal(i.cpu(), i_ref)
        assert torch.equal(d.cpu(), d_ref)


def test_knn_kitti_shaped_batch32_properties(cuda):
    """B=32, N=8192, S=2048, K=32: distances ascending, self-match first, no repeated index;
    oracle parity on one cloud."""
    pc1, _, _, _ = synthetic.kitti_like_pair(78, 8192, 2)
    x = torch.from_numpy(np.tile(pc1[:, :, :3], (16, 1, 1))).contiguous()
    x = x * (1 + torch.arange(32).reshape(32, 1, 1) * 1e-3)
    q = x[:, :2048].contiguous()
    d, i = E.knn_point(32, g(x, cuda), g(q, cuda), return_dist=True)
    d, i = d.cpu(), i.cpu()
    assert (d[:, :, 1:] >= d[:, :, :-1]).all()
    assert (i[:, :, 0] == torch.arange(2048).reshape(1, -1)).all()
    assert (torch.sort(i, dim=2)[0].diff(dim=2) > 0).all()
    d_ref, i_ref = O.knn_point_with_dist(32, x[31:32].contiguous(), q[31:32].contiguous())
    assert torch.equal(i[31:32], i_ref) and torch.equal(d[31:32], d_ref)


def test_knn_rejects_bad_arguments(cuda):
    xyz = rand_cloud(1, 1, 10).to(cuda)
    with pytest.raises(RuntimeError):
        E.knn_point(11, xyz, xyz)          # nsample > n
    with pytest.raises(RuntimeError):
        E.knn_point(65, rand_cloud(1, 1, 100).to(cuda), xyz)  # nsample > 64
    with pytest.raises(RuntimeError):
        E.knn_point(4, xyz.double(), xyz)  # dtype check, like CHECK_IS_FLOAT
    with pytest.raises(RuntimeError):
        E.group_points(xyz.cpu().transpose(1, 2).contiguous(), torch.zeros(1, 2, 2, dtype=torch.int32))


# ---------------------------------------------------------------- quaternion warp
def test_quat_warp(cuda):
    from oracle import model as M
    gen = torch.Generator().manual_seed(3)
    xyz = (torch.rand(4, 3, 2048, generator=gen) * 2 - 1) * 30
    q = torch.randn(4, 4, 1, generator=gen)
    q = q / q.norm(dim=1, keepdim=True)
    q[3] *= 1.7  # not normalised: exercises the 1/(|q|^2+1e-10) factor
    t = torch.randn(4, 3, 1, generator=gen)
    ref = M.warp(xyz, q, t)
    out = E.quat_warp(g(xyz, cuda), g(q, cuda), g(t, cuda)).cpu()
    torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-5)
    # known answer: rotate (1,0,0) by 90 deg about z, then translate
    one = torch.tensor([[[1.0], [0.0], [0.0]]])
    qz = torch.tensor([[[np.cos(np.pi / 4)], [0.0], [0.0], [np.sin(np.pi / 4)]]], dtype=torch.float32)
    tt = torch.tensor([[[1.0], [2.0], [3.0]]])
    got = E.quat_warp(one.to(cuda), qz.to(cuda), tt.to(cuda)).cpu().flatten()
    torch.testing.assert_close(got, torch.tensor([1.0, 3.0, 3.0]), rtol=0, atol=1e-6)


@pytest.mark.parametrize("k,n,s", [(32, 8192, 2048), (6, 2048, 2048), (16, 1024, 256), (1, 513, 277),
                                   (64, 16384, 300), (8, 700, 1500)])
def test_knn_pruned_equals_exhaustive(cuda, k, n, s):
    """The spatially pruned search (256 <= n <= 16384, >= 256 queries) returns exactly what the exhaustive
    kernel returns, on KITTI-shaped (strongly non-uniform) clouds and with duplicated points.  The plan query
    confirms that the first call of every case searches a structure (K = 64: knn_pruned_kernel, the others a rows
    kernel); tests/test_gpu_knn_variants.py pins every form."""
    plan = E.knn_point_plan(2, n, s, k)
    assert plan["kernel"] != "exhaustive" and plan["build_r"] > 0, plan
    assert plan["kernel"] == ("pruned" if k > 32 else "rows"), plan
    pc1, _, _, _ = synthetic.kitti_like_pair(90 + k, 8192, 2)
    base = torch.from_numpy(np.ascontiguousarray(pc1[:, :, :3]))
    reps = (n + 8191) // 8192
    x = base.repeat(1, reps, 1)[:, :n].contiguous()          # n > 8192: exact duplicates
    q = (x[:, torch.randperm(n, generator=torch.Generator().manual_seed(k))[:s] % n] + 0.05).contiguous() \
        if s <= n else (torch.rand(2, s, 3) * 40 - 20)
    x, q = x.to(cuda), q.to(cuda)
    d1, i1 = E.knn_point(k, x, q, return_dist=True)
    d0, i0 = E.knn_point(k, x, q, return_dist=True, exhaustive=True)
    assert torch.equal(i1, i0)
    assert torch.equal(d1, d0)


# the rows form every case reaches (knn_rows_kernel<L, R>, asserted through the plan query)
KNN_ROWS_SHAPES = [(4, 2000, 523, (16, 3)), (6, 2000, 523, (16, 3)), (16, 5000, 1201, (16, 9)), (32, 5000, 1201, (32, 3)),
                   (8, 16384, 600, (16, 17)), (32, 16000, 513, (32, 9)), (1, 600, 700, (16, 2)), (12, 513, 512, (16, 2))]


@pytest.mark.parametrize("k,n,s", [c[:3] for c in KNN_ROWS_SHAPES])
def test_knn_rows_kernel_ties_and_ragged_shapes(cuda, k, n, s):
    """K <= 32 with >= 256 queries runs several queries per wave (csrc/knn.hip: knn_rows_kernel, L = 16 / 32 lanes per
    query): integer-lattice clouds (exact distance ties at every rank, duplicated points: lower index first), query
    counts that are not a multiple of the queries per wave / workgroup, n up to 16384, against the oracle -- indices
    AND keys bit for bit.  Each case asserts the rows form it reaches; tests/knn_cases.py holds the table that covers
    every form and both sides of every register-count boundary."""
    plan = E.knn_point_plan(2, n, s, k)
    assert (plan["kernel"], (plan["L"], plan["R"])) == ("rows", dict((c[:3], c[3]) for c in KNN_ROWS_SHAPES)[(k, n, s)]), plan
    gen = torch.Generator().manual_seed(k * 100 + n)
    xyz = torch.randint(-7, 8, (2, n, 3), generator=gen).float()
    xyz[1] = (torch.rand(n, 3, generator=gen) * 2 - 1) * 25            # one lattice cloud, one random cloud
    xyz[1, 100:140] = xyz[1, 60:100]                                  # + exact duplicates
    new_xyz = torch.stack((xyz[0, torch.randperm(n, generator=gen)[:s] % n] if s <= n else xyz[0, torch.randint(0, n, (s,), generator=gen)],
                           (torch.rand(s, 3, generator=gen) * 2 - 1) * 25)).contiguous()
    d_ref, i_ref = O.knn_point_with_dist(k, xyz, new_xyz)
    d, i = E.knn_point(k, g(xyz, cuda), g(new_xyz, cuda), return_dist=True)
    assert torch.equal(i.cpu(), i_ref)
    assert torch.equal(d.cpu(), d_ref)


def test_kitti_transform_filter_and_sampling(cuda):
    """the on-device transform + filter is the source-order host model (tests/frontend_model.py) bit
    for bit, coordinates and mask, with no row excused; against the NumPy restatement of the dataset code (a BLAS matmul,
    another summation order) it is identical up to one fp32 ulp with the same mask away from the thresholds; and both
    sampling modes return npoints survivors."""
    import frontend_model
    from oracle.preprocess import transform_filter as ref_tf
    from pwclonet_pylidarslam_amd import preprocess
    rng = np.random.default_rng(12)
    n = 123457
    pts = np.concatenate([rng.uniform(-70, 70, (n, 2)), rng.uniform(-3, 2, (n, 1)), rng.uniform(0, 1, (n, 1))],
                         axis=1).astype(np.float32)
    tr = np.array([[4.3e-4, -0.99997, -8.0e-3, -1.2e-2], [-7.2e-3, 8.1e-3, -0.99994, -5.4e-2],
                   [0.99997, 4.9e-4, -7.2e-3, -0.292]])                       # KITTI-like calibration
    q, keep = ref_tf(pts, tr)
    xyz, k = preprocess.transform_filter(torch.from_numpy(pts).to(cuda), tr)
    got = xyz.cpu().numpy()
    model_words, model_keep = frontend_model.kitti_row(pts, tr)
    assert np.array_equal(got.view(np.int32), model_words)
    assert np.array_equal(k.cpu().numpy(), model_keep.astype(np.int32))
    ref32 = q.astype(np.float32)
    ulp = np.abs(got.view(np.int32).astype(np.int64) - ref32.view(np.int32).astype(np.int64))
    assert ulp.max() <= 1 and (ulp > 0).mean() < 1e-3
    mism = np.nonzero(k.cpu().numpy().astype(bool) != keep)[0]
    assert len(mism) == 0 or all(np.min(np.abs(np.abs(q[i, [0, 2]]) - 30)) < 1e-9 or abs(q[i, 1] - 1.1) < 1e-9
                                 for i in mism)
    gen = torch.Generator(device=cuda).manual_seed(5)
    cloud = preprocess.kitti_frame_to_cloud(torch.from_numpy(pts).to(cuda), tr, 8192, generator=gen)
    assert cloud.shape == (8192, 3)
    kept = q[keep].astype(np.float32)
    assert set(map(tuple, cloud.cpu().numpy().round(4))) <= set(map(tuple, np.concatenate((kept, got[k.cpu().numpy() > 0])).round(4)))
    assert len(np.unique(cloud.cpu().numpy(), axis=0)) == 8192          # drawn without replacement
    fps_cloud = preprocess.kitti_frame_to_cloud(torch.from_numpy(pts).to(cuda), tr, 2048, sample="fps")
    assert fps_cloud.shape == (2048, 3) and len(np.unique(fps_cloud.cpu().numpy(), axis=0)) == 2048
    cand = torch.from_numpy(got[k.cpu().numpy() > 0]).unsqueeze(0).contiguous()
    assert torch.equal(fps_cloud.cpu(), cand[0][O.furthest_point_sampling(cand, 2048)[0].long()])


def _raw_frames(seed, b, n):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-60, 60, (b, n, 2)), rng.uniform(-2.5, 2, (b, n, 1)),
                           rng.uniform(0, 1, (b, n, 1))], axis=2).astype(np.float32)


def test_kitti360_filter_compaction_and_batched_sampling(cuda):
    """SURVEY section 8 f2, KITTI-360 variant + batching: mask and coordinates bitwise equal to the NumPy
    restatement of filter_pcd; the per-frame stable compaction equals boolean indexing, zero padded; the
    batched furthest point sampling of the packed frames equals the oracle's sampler on each frame's survivors
    (padding changes nothing: zero rows are skipped and bs = 512 for every N >= 512)."""
    from oracle.preprocess import kitti360_filter as ref_filter
    from pwclonet_pylidarslam_amd import preprocess
    b, n, m = 3, 30011, 384
    pts = _raw_frames(31, b, n)
    pts[1, :, :2] *= 2.0                                  # fewer survivors in frame 1
    pts[2, 100:200, :3] = pts[2, 0:100, :3]               # duplicated rows survive in order
    dev = torch.from_numpy(pts).to(cuda)
    xyz, keep = preprocess.kitti360_filter(dev, 35.0)
    refs = [ref_filter(pts[f], 35.0) for f in range(b)]
    for f in range(b):
        assert np.array_equal(xyz[f].cpu().numpy().view(np.int32), refs[f][0].view(np.int32))
        assert np.array_equal(keep[f].cpu().numpy().astype(bool), refs[f][1])
    packed, counts = preprocess.compact(xyz, keep)
    assert packed.shape == (b, n, 3)
    for f in range(b):
        kept = refs[f][0][refs[f][1]]
        assert int(counts[f]) == len(kept)
        assert np.array_equal(packed[f, :len(kept)].cpu().numpy(), kept)
        assert not packed[f, len(kept):].any()
    small, c2 = preprocess.compact(xyz, keep, cap=5000)   # survivors beyond cap are dropped, counts clipped
    assert small.shape == (b, 5000, 3) and c2.tolist() == [min(int(c), 5000) for c in counts]
    assert torch.equal(small, packed[:, :5000])
    clouds, counts2 = preprocess.frames_to_clouds(dev, m, dataset="kitti360", near_threshold=35.0)
    assert torch.equal(counts2, counts) and clouds.shape == (b, m, 3)
    for f in range(b):
        kept = torch.from_numpy(np.ascontiguousarray(refs[f][0][refs[f][1]])).unsqueeze(0)
        ref_idx = O.furthest_point_sampling(kept, m)[0].long()
        assert torch.equal(clouds[f].cpu(), kept[0][ref_idx])
    single, _ = preprocess.kitti360_filter(dev[0], 35.0)  # (n,4) form
    assert torch.equal(single, xyz[0])


def test_kitti_batched_frames_to_clouds(cuda):
    """Batched KITTI-odometry front end (one calibration for the batch) equals the per-frame path."""
    from pwclonet_pylidarslam_amd import preprocess
    tr = np.array([[4.3e-4, -0.99997, -8.0e-3, -1.2e-2], [-7.2e-3, 8.1e-3, -0.99994, -5.4e-2],
                   [0.99997, 4.9e-4, -7.2e-3, -0.292]])
    pts = _raw_frames(32, 2, 20000)
    dev = torch.from_numpy(pts).to(cuda)
    clouds, counts = preprocess.frames_to_clouds(dev, 256, dataset="kitti", tr=tr)
    for f in range(2):
        one = preprocess.kitti_frame_to_cloud(dev[f], tr, 256, sample="fps")
        assert torch.equal(clouds[f], one)
        assert int(counts[f]) == int(preprocess.transform_filter(dev[f], tr)[1].sum())


@pytest.mark.parametrize("b,c,n,s,k", [(2, 16, 500, 300, 8), (3, 67, 1024, 2048, 4), (1, 3, 64, 256, 32)])
def test_deterministic_scatter_grad(cuda, b, c, n, s, k):
    """Atomics-free backward of grouping / gather: same sums as the oracle within fp32
    summation order, bit-identical across runs, and reachable through the autograd Functions."""
    from pwclonet_pylidarslam_amd.pointnet2_ops import pointnet2_utils as PU
    gen = torch.Generator().manual_seed(b * 1000 + n)
    idx = torch.randint(0, n, (b, s, k), generator=gen, dtype=torch.int32)
    go = torch.randn(b, c, s, k, generator=gen)
    ref = O.group_points_grad(go, idx, n)
    out1 = E.scatter_grad_deterministic(g(go, cuda), g(idx, cuda), n)
    out2 = E.scatter_grad_deterministic(g(go, cuda), g(idx, cuda), n)
    assert torch.equal(out1, out2)
    torch.testing.assert_close(out1.cpu(), ref, rtol=1e-5, atol=1e-5)
    idx1 = idx[:, :, 0].contiguous()                                   # gather form (B,M)
    go1 = go[:, :, :, 0].contiguous()
    torch.testing.assert_close(E.scatter_grad_deterministic(g(go1, cuda), g(idx1, cuda), n).cpu(),
                               O.gather_points_grad(go1, idx1, n), rtol=1e-5, atol=1e-5)
    PU.deterministic_grads(True)
    try:
        feat = torch.randn(b, c, n, generator=gen).to(cuda).requires_grad_(True)
        PU.grouping_operation(feat, g(idx, cuda)).mul(g(go, cuda)).sum().backward()
        assert torch.equal(feat.grad, out1)
    finally:
        PU.deterministic_grads(False)


@pytest.mark.parametrize("b,c,n,s,k", [(2, 16, 500, 300, 8), (3, 67, 1024, 2048, 4), (1, 3, 64, 257, 3), (2, 3, 8192, 2048, 32),
                                       (2, 128, 5000, 64, 16)])
def test_group_concat_equals_cat_of_grouped(cuda, b, c, n, s, k):
    """The concatenated input of a shared MLP (P2/pointnet2_modules.py:222-230, PW/costvolume.py:134) built with the
    grouping kernel writing its channel slice directly: bit-identical to ``torch.cat`` of ``grouping_operation`` forward,
    and its backward (atomic and atomics-free form) equals the oracle's group_points_grad of the gradient's slice."""
    from pwclonet_pylidarslam_amd.pointnet2_ops import pointnet2_utils as PU
    gen = torch.Generator().manual_seed(b * 77 + n + k)
    idx = torch.randint(0, n, (b, s, k), generator=gen, dtype=torch.int32)
    feat = torch.randn(b, c, n, generator=gen)
    other = torch.randn(b, 5, n, generator=gen)
    dense = torch.randn(b, 3, s, k, generator=gen)
    centre = torch.randn(b, 7, s, generator=gen)
    go = torch.randn(b, 3 + c + 7 + 5, s, k, generator=gen)
    want = torch.cat((dense, O.group_points(feat, idx), centre.unsqueeze(3).expand(-1, -1, -1, k),
                      O.group_points(other, idx)), dim=1)
    for det in (False, True):
        PU.deterministic_grads(det)
        try:
            f, o, d, ce = (t.to(cuda).requires_grad_(True) for t in (feat, other, dense, centre))
            got = PU.group_concat(g(idx, cuda), ("t", d), ("g", f), ("t", ce.unsqueeze(3).expand(-1, -1, -1, k)), ("g", o))
            assert torch.equal(got.cpu(), want)
            got.backward(g(go, cuda))
            torch.testing.assert_close(f.grad.cpu(), O.group_points_grad(go[:, 3:3 + c].contiguous(), idx, n),
                                       rtol=1e-5, atol=1e-5)
            torch.testing.assert_close(o.grad.cpu(), O.group_points_grad(go[:, 10 + c:].contiguous(), idx, n),
                                       rtol=1e-5, atol=1e-5)
            assert torch.equal(d.grad.cpu(), go[:, :3])
            torch.testing.assert_close(ce.grad.cpu(), go[:, 3 + c:10 + c].sum(3), rtol=1e-5, atol=1e-5)
            if det:
                assert torch.equal(f.grad, E.scatter_grad_deterministic(g(go[:, 3:3 + c].contiguous(), cuda), g(idx, cuda), n))
        finally:
            PU.deterministic_grads(False)
    with pytest.raises(ValueError):
        E.group_points_into(g(feat, cuda), g(idx, cuda), torch.empty(b, c, s, k, device=cuda), 1)


@pytest.mark.parametrize("b,n,s,k,c1,c2,same", [(2, 500, 300, 6, 16, 8, False), (3, 256, 256, 4, 64, 64, True), (1, 64, 33, 5, 3, 1, False),
                                                 (2, 2048, 2048, 6, 32, 32, False), (2, 40, 40, 32, 128, 7, True)])
def test_cost_volume_inputs_as_parts_of_the_concatenation(cuda, b, n, s, k, c1, c2, same):
    """group_concat parts "geo" (the 10-channel geometry encoding of PW/costvolume.py:92-105) and "c" (torch.tile of the
    centre features, :95) against the reference's chain of torch ops evaluated by torch on the GPU: forward bit for bit
    (same fp32 expressions, no fused multiply-add), backward against a float64 evaluation of the same chain at 1e-5 of
    each gradient's scale -- including the second aggregate's case where centres and neighbours are the same cloud
    (``same``: both roles receive a gradient and autograd adds them)."""
    from pwclonet_pylidarslam_amd.pointnet2_ops import pointnet2_utils as PU
    gen = torch.Generator().manual_seed(b * 31 + n + k)
    src = torch.randn(b, 3, n, generator=gen) * 10
    centre = src.clone() if same else torch.randn(b, 3, s, generator=gen) * 10
    assert centre.shape[2] == s
    idx = torch.randint(0, n, (b, s, k), generator=gen, dtype=torch.int32)
    if same:
        idx[:, :, 0] = torch.arange(s, dtype=torch.int32)          # the point itself: |q - p| = sqrt(1e-20)
    pf = torch.randn(b, c1, s, generator=gen)
    qf = torch.randn(b, c2, n, generator=gen)
    go = torch.randn(b, 10 + c1 + c2, s, k, generator=gen)

    def chain(cx, sx, pfeat, qfeat, dt):
        gather = lambda t: torch.gather(t.unsqueeze(2).expand(-1, -1, s, -1), 3,
                                        idx.to(t.device).long().unsqueeze(1).expand(-1, t.shape[1], -1, -1))
        q = gather(sx)
        p = cx.unsqueeze(3).expand(-1, -1, -1, k)
        diff = q - p
        euc = torch.sqrt(torch.sum(torch.square(diff), dim=1, keepdim=True) + 1e-20)
        return torch.cat((p, q, diff, euc, pfeat.unsqueeze(3).expand(-1, -1, -1, k), gather(qfeat)), dim=1)

    want = chain(centre.to(cuda), src.to(cuda), pf.to(cuda), qf.to(cuda), torch.float32)
    l64 = [t.double().requires_grad_(True) for t in ((centre,) if same else (centre, src))] + \
          [pf.double().requires_grad_(True), qf.double().requires_grad_(True)]
    c64, s64 = (l64[0], l64[0]) if same else (l64[0], l64[1])
    chain(c64, s64, l64[-2], l64[-1], torch.float64).backward(go.double())

    def run():
        leaves = [t.to(cuda).requires_grad_(True) for t in ((centre,) if same else (centre, src))] + \
                 [pf.to(cuda).requires_grad_(True), qf.to(cuda).requires_grad_(True)]
        cx, sx = (leaves[0], leaves[0]) if same else (leaves[0], leaves[1])
        got = PU.group_concat(g(idx, cuda), ("geo", cx, sx), ("c", leaves[-2]), ("g", leaves[-1]))
        assert torch.equal(got, want)
        got.backward(go.to(cuda))
        return [t.grad for t in leaves]

    for det in (False, True):                  # fp32 atomics / the atomics-free sorted scatter
        PU.deterministic_grads(det)
        try:
            grads = run()
            for a_, r_ in zip(grads, l64):
                scale = r_.grad.abs().max().item()
                assert (a_.cpu().double() - r_.grad).abs().max().item() <= 1e-5 * scale + 1e-12, (a_.shape, scale, det)
            if det:
                for a_, b_ in zip(grads, run()):
                    assert torch.equal(a_, b_)
        finally:
            PU.deterministic_grads(False)
    # gradient not wanted for the neighbour coordinates (the pyramid's clouds): no scatter, same centre gradient
    cx2 = centre.to(cuda).requires_grad_(True)
    PU.group_concat(g(idx, cuda), ("geo", cx2, src.to(cuda))).backward(go[:, :10].contiguous().to(cuda))
    if not same:
        cx3 = centre.to(cuda).requires_grad_(True)
        sx3 = src.to(cuda).requires_grad_(True)
        PU.group_concat(g(idx, cuda), ("geo", cx3, sx3)).backward(go[:, :10].contiguous().to(cuda))
        assert torch.equal(cx2.grad, cx3.grad)


@pytest.mark.parametrize("b,n,s,k", [(2, 500, 300, 8), (1, 64, 33, 5), (2, 8192, 2048, 32)])
def test_grouped_coordinates_relative_to_their_centres_as_a_part(cuda, b, n, s, k):
    """group_concat part "diff" = grouping_operation(xyz) - centres (P2/pointnet2_modules.py:215-218, 485-488): forward bit
    for bit against the two torch ops, both gradients (fp32 atomics and the atomics-free scatter) against the oracle's
    group_points_grad / a float64 sum."""
    from pwclonet_pylidarslam_amd.pointnet2_ops import pointnet2_utils as PU
    gen = torch.Generator().manual_seed(b + n + k)
    src = torch.randn(b, 3, n, generator=gen) * 10
    centre = torch.randn(b, 3, s, generator=gen) * 10
    idx = torch.randint(0, n, (b, s, k), generator=gen, dtype=torch.int32)
    go = torch.randn(b, 3, s, k, generator=gen)
    want = O.group_points(src, idx) - centre.unsqueeze(3)
    for det in (False, True):
        PU.deterministic_grads(det)
        try:
            cx, sx = centre.to(cuda).requires_grad_(True), src.to(cuda).requires_grad_(True)
            got = PU.group_concat(g(idx, cuda), ("diff", cx, sx))
            assert torch.equal(got.cpu(), want)
            got.backward(go.to(cuda))
            torch.testing.assert_close(sx.grad.cpu(), O.group_points_grad(go, idx, n), rtol=1e-5, atol=1e-5)
            torch.testing.assert_close(cx.grad.cpu().double(), -go.double().sum(3), rtol=1e-5, atol=1e-5)
        finally:
            PU.deterministic_grads(False)


@pytest.mark.parametrize("shape", [(4, 8, 300, 7), (8, 16, 2048, 32), (2, 64, 1, 5), (3, 5, 1000), (32, 128, 64, 8)])
@pytest.mark.parametrize("affine,relu", [(True, False), (False, False), (True, True)])
def test_batchnorm_train_kernels(cuda, shape, affine, relu):
    """training-mode BatchNorm on the HIP kernels equals a float64 evaluation of
    torch.nn.functional.batch_norm(training=True) -- output, running statistics, num_batches_tracked, and the
    gradients of input / weight / bias -- and is what the pytorch_utils BatchNorm wrappers run in train mode."""
    from pwclonet_pylidarslam_amd import batchnorm as hip_bn
    from pwclonet_pylidarslam_amd.pointnet2_ops import pytorch_utils as PT
    gen = torch.Generator().manual_seed(sum(shape))
    C = shape[1]
    x = (torch.randn(*shape, generator=gen) * 1.7 + 0.6)
    go = torch.randn(*shape, generator=gen)
    cls = torch.nn.BatchNorm2d if len(shape) == 4 else torch.nn.BatchNorm1d
    ref = cls(C, affine=affine, momentum=0.1).double().train()
    bn = cls(C, affine=affine, momentum=0.1).to(cuda).train()
    with torch.no_grad():
        for m in (ref, bn):
            m.running_mean.copy_(torch.linspace(-0.5, 0.5, C))
            m.running_var.copy_(torch.linspace(0.5, 1.5, C))
            if affine:
                m.weight.copy_(torch.linspace(0.7, 1.3, C))
                m.bias.copy_(torch.linspace(-0.2, 0.2, C))
    xr = x.double().requires_grad_(True)
    pre = ref(xr)
    yr = torch.relu(pre) if relu else pre
    # fused ReLU: the mask is decided in fp32; keep the comparison away from outputs within rounding of zero
    if relu:
        go = go * (pre.detach().abs() > 1e-4).float()
    yr.backward(go.double())
    xg = x.to(cuda).requires_grad_(True)
    assert hip_bn.supported(xg, bn)
    yg = hip_bn.batch_norm_train(xg, bn, relu=relu)
    yg.backward(go.to(cuda))

    def close(a, b, tol):
        b = b.float()
        assert (a.cpu() - b).abs().max() <= tol * max(1.0, float(b.abs().max())), float((a.cpu() - b).abs().max())
    close(yg.detach(), yr.detach(), 2e-6)
    close(bn.running_mean, ref.running_mean, 1e-6)
    close(bn.running_var, ref.running_var, 1e-6)
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked) == 1
    close(xg.grad, xr.grad, 5e-6)
    if affine:
        close(bn.weight.grad, ref.weight.grad, 2e-6)
        close(bn.bias.grad, ref.bias.grad, 2e-6)
    if len(shape) == 4 and affine and not relu:   # the wrapper module takes this path in train mode and torch's in eval mode
        w = PT.BatchNorm2d(C).to(cuda)
        w.load_state_dict({"bn." + k: v for k, v in bn.state_dict().items()})
        w.train()
        y2 = w(x.to(cuda))
        w.eval()
        y3 = w(x.to(cuda))
        assert int(w[0].num_batches_tracked) == 2 and y2.shape == y3.shape
        bn.eval()
        ref2 = bn(x.to(cuda))             # eval with the statistics after ONE update; w has had two
        assert not torch.equal(ref2, y3)


def test_sample_and_gather_chain_on_module_path(cuda):
    """pointnet2_utils.sample_and_gather (what the SA modules call): a pyramid sampled through the chain record that
    travels on the returned tensors equals separate furthest_point_sample + gather_operation calls at every level --
    on lidar-shaped clouds, on an integer lattice (exact ties -> fallback flag) and after an in-place edit of a level's
    coordinates (record dropped: version counter)."""
    from pwclonet_pylidarslam_amd.pointnet2_ops import pointnet2_utils as PU
    pc1, _, _, _ = synthetic.kitti_like_pair(321, 8192, 3)
    lattice = torch.stack(torch.meshgrid(torch.arange(16.), torch.arange(16.), torch.arange(8.), indexing="ij"),
                          dim=-1).reshape(1, 2048, 3).repeat(2, 1, 1) + 1.0

    def plain(x, m):
        idx = PU.furthest_point_sample(x, m)
        return PU.gather_operation(x.transpose(1, 2).contiguous(), idx).transpose(1, 2).contiguous()

    for cloud, levels in ((torch.from_numpy(pc1[:, :, :3].copy()).float(), (2048, 1024, 256, 64)),
                          (lattice, (1024, 512, 256, 64))):
        x = cloud.to(cuda).contiguous()
        chained, ref = x, x.clone()
        for lvl, m in enumerate(levels):
            chained = PU.sample_and_gather(chained, m)
            ref = plain(ref.clone(), m)                       # clone: no record attached
            assert torch.equal(chained, ref), (lvl, m)
            assert hasattr(chained, PU._CHAIN_ATTR)
        # the last level of frame-1's pyramid is sampled twice in PWCLO-Net (flow_feature_encoding): same record
        assert torch.equal(PU.sample_and_gather(chained, 16), plain(ref.clone(), 16))
    # in-place edit invalidates the record: the next level must be sampled from the edited coordinates
    lvl1 = PU.sample_and_gather(torch.from_numpy(pc1[:1, :, :3].copy()).float().to(cuda).contiguous(), 2048)
    lvl1[:, :100] += 5.0
    assert torch.equal(PU.sample_and_gather(lvl1, 1024), plain(lvl1.clone(), 1024))
