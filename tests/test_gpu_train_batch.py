"""GPU tests of the device-side training batch builder (``batches.TrainBatchBuilder``; run with ``-m gpu``): the kernels of
csrc/train_batch.hip against the NumPy host model (tests/train_batch_model.py, written from DESIGN.md section 13) and
against the existing filter kernels.  Selection (indices, survivor counts) and every unaugmented coordinate are compared BIT
FOR BIT; what passes through libm in fp64 on both sides (the drawn parameters, the moved coordinates, the ground truth) to
the bounds the two roundings allow: 1 fp32 ulp, 1e-12 relative in fp64."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_batch_model as model                                             # noqa: E402

from pwclonet_pylidarslam_amd import preprocess, synthetic                    # noqa: E402
from pwclonet_pylidarslam_amd.batches import TrainBatchBuilder, pad_pairs     # noqa: E402

pytestmark = pytest.mark.gpu
VELO_TO_CAM = np.array([[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0], [1.0, 0.0, 0.0, 0.0]])


def _t_diff(B, seed):
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    T = np.tile(np.eye(4), (B, 1, 1))
    for b in range(B):
        T[b, :3, :3] = Rotation.from_rotvec(rng.normal(0, 0.03, 3)).as_matrix()
        T[b, :3, 3] = rng.normal(0, 0.8, 3)
    return T


def _case(B, n_azimuth=512, seed=21, regimes=True):
    """B pairs of consecutive raw sweeps (velodyne frame, scan order, unequal row counts).  With ``regimes`` and B >= 8:
    pair 2 is cut to a few hundred rows (0 < count < npoints for npoints = 1024), pair 5's pc2 lies entirely outside the
    range box (count == 0) and pair 6's pc1 likewise; the others have plenty of survivors."""
    frames, _q, _t = synthetic.raw_sweep_sequence(seed, frames=B + 1, n_azimuth=n_azimuth)
    pairs = [(frames[b].copy(), frames[b + 1].copy()) for b in range(B)]
    if regimes and B >= 8:
        pairs[2] = (pairs[2][0][:700], pairs[2][1][:650])
        far = pairs[5][1].copy()
        far[:, :2] += 100.0
        pairs[5] = (pairs[5][0], far)
        far = pairs[6][0].copy()
        far[:, :2] -= 100.0
        pairs[6] = (far, pairs[6][1][:-37])
    sweeps, lengths = pad_pairs(pairs)
    return sweeps, lengths, _t_diff(B, seed + 1)


def _ulps(a, b):
    """Distance of two float32 arrays in units in the last place (of the ordered integer representation)."""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def _builder(dataset, B, npoints, capacity, **kw):
    return TrainBatchBuilder(B, dataset=dataset, npoints=npoints, capacity=capacity,
                             tr=VELO_TO_CAM if dataset == "kitti" else None, **kw)


def _existing_filter(dataset, frame):
    if dataset == "kitti":
        return preprocess.transform_filter(frame, VELO_TO_CAM)
    return preprocess.kitti360_filter(frame, 30.0)


@pytest.mark.parametrize("dataset", ["kitti", "kitti360"])
@pytest.mark.parametrize("B", [1, 8])
def test_batch_against_host_model(cuda, dataset, B):
    npoints, seed, step = 1024, 77, 3
    sweeps, lengths, Td = _case(B)
    assert sweeps.shape[2] < 40000 and any(int(a) != int(b) for a, b in lengths)       # R < capacity, unequal lengths
    bld = _builder(dataset, B, npoints, 40000, seed=seed)
    bld.set_step(step)
    dsweeps = sweeps.to(cuda)
    x1, x2, gt = bld.build(dsweeps, lengths, torch.from_numpy(Td))
    torch.cuda.synchronize()
    assert x1.shape == (B, 3, npoints) and x1.is_contiguous() and gt.shape == (B, 7) and bld.step_index() == step + 1
    tr = VELO_TO_CAM if dataset == "kitti" else None
    ref = model.build(dataset, sweeps.numpy(), lengths.numpy(), Td, npoints, seed, step, tr=tr)

    # selection: bit-equal
    counts = bld.survivor_counts().cpu().numpy()
    assert np.array_equal(counts, ref["counts"]), (counts, ref["counts"])
    if B >= 8:
        assert 0 < counts[4] < npoints and 0 < counts[5] < npoints and counts[11] == 0 and counts[12] == 0
        assert counts[0] >= npoints and counts[10] >= npoints
    idx = bld.indices().cpu().numpy()
    assert np.array_equal(idx, ref["indices"]), np.nonzero((idx != ref["indices"]).any(axis=1))[0]

    # pc1 side == the existing filter kernels' coordinates gathered at the indices, bit for bit
    plain = (x2 if dataset == "kitti" else x1).cpu()
    for b in range(B):
        n = int(lengths[b].min())
        xyz, keep = _existing_filter(dataset, dsweeps[b, 0, :n])
        assert int(keep.sum()) == counts[2 * b]
        want = xyz[torch.from_numpy(idx[2 * b]).long().to(cuda)].t().cpu()
        assert torch.equal(plain[b], want), b
    assert np.array_equal(plain.numpy(), ref["xyz_f2" if dataset == "kitti" else "xyz_f1"])

    # drawn parameters: both sides compute in fp64 and round once
    aug = bld.aug_params().cpu().numpy()
    d = _ulps(aug, ref["aug"])
    print("aug_params: max %d ulp from the host model" % d.max())
    assert d.max() <= 1
    assert np.all(np.abs(aug) <= np.array(model.AUG_CLIP, dtype=np.float32))

    # the rest with the DEVICE's parameters fed to the model
    ref = model.build(dataset, sweeps.numpy(), lengths.numpy(), Td, npoints, seed, step, tr=tr, aug=aug)
    moved, want = (x1 if dataset == "kitti" else x2).cpu().numpy(), ref["xyz_f1" if dataset == "kitti" else "xyz_f2"]
    d = _ulps(moved, want)
    print("augmented coordinates: max %d ulp" % d.max())
    assert d.max() <= 1
    tg = bld.t_gt().cpu().numpy()
    rel = np.abs(tg - ref["t_gt"]).reshape(B, -1).max(axis=1) / np.abs(ref["t_gt"]).reshape(B, -1).max(axis=1)
    print("t_gt: max relative difference %.2e" % rel.max())
    assert rel.max() <= 1e-12
    g = gt.cpu().numpy()
    dq = np.abs(g[:, 3:].astype(np.float64) - ref["gt"][:, 3:]).max()
    tscale = np.maximum(np.abs(ref["gt"][:, :3]).max(axis=1), 1.0).astype(np.float32)
    dt = (np.abs(g[:, :3].astype(np.float64) - ref["gt"][:, :3]).max(axis=1) / np.spacing(tscale)).max()
    print("gt: quaternion max abs difference %.2e, translation %.2f ulp of max(|t|, 1)" % (dq, dt))
    assert dq <= 2.0 ** -23 and dt <= 1.0
    assert np.abs(np.linalg.norm(g[:, 3:], axis=1) - 1).max() < 1e-6

    # build(aug=...) uses the given parameters
    given = torch.from_numpy(ref["aug"][::-1].copy()).to(cuda)
    bld.set_step(step)
    y1, y2, _ = bld.build(dsweeps, lengths, torch.from_numpy(Td), aug=given)
    assert torch.equal(bld.aug_params(), given) and torch.equal(bld.indices().cpu(), torch.from_numpy(idx))


def test_full_size_selection_against_host_model(cuda):
    """npoints = 8192 on raw-sized sweeps (the 64 KiB LDS selection), both datasets' row bodies."""
    sweeps, lengths, Td = _case(2, n_azimuth=2048, seed=5, regimes=False)
    assert sweeps.shape[2] > 60000
    for dataset in ("kitti", "kitti360"):
        bld = _builder(dataset, 2, 8192, 131072, seed=(1 << 63) + 12345)
        bld.set_step((1 << 32) + 6)                       # the low 32 bits of the step enter the counter
        bld.build(sweeps.to(cuda), lengths.to(cuda), torch.from_numpy(Td).to(cuda))
        ref = model.build(dataset, sweeps.numpy(), lengths.numpy(), Td, 8192, (1 << 63) + 12345, 6,
                          tr=VELO_TO_CAM if dataset == "kitti" else None)
        assert np.array_equal(bld.survivor_counts().cpu().numpy(), ref["counts"]) and ref["counts"].min() >= 8192
        assert np.array_equal(bld.indices().cpu().numpy(), ref["indices"])
        assert bld.step_index() == (1 << 32) + 7


@pytest.mark.parametrize("dataset", ["kitti", "kitti360"])
def test_without_augmentation(cuda, dataset):
    B, npoints = 8, 1024
    sweeps, lengths, Td = _case(B)
    bld = _builder(dataset, B, npoints, 40000, seed=3, augment=False)
    dsweeps = sweeps.to(cuda)
    x1, x2, gt = bld.build(dsweeps, lengths, torch.from_numpy(Td[:, :3]))      # (B,3,4) is taken too
    assert torch.equal(bld.t_gt().cpu(), torch.from_numpy(Td)) and not bld.aug_params().any()
    idx = bld.indices()
    pc2 = x1 if dataset == "kitti" else x2
    for b in range(B):
        n = int(lengths[b].min())
        xyz, _ = _existing_filter(dataset, dsweeps[b, 1, :n])
        assert torch.equal(pc2[b], xyz[idx[2 * b + 1].long()].t()), b           # unaugmented: a bit-equal gather
    g = gt.cpu().numpy()
    for b in range(B):
        _, _, want = model.pose(dataset, Td[b], None)
        assert np.abs(g[b, 3:] - want[3:]).max() <= 2.0 ** -23 and np.array_equal(g[b, :3], want[:3])


def test_replay_steps_seeds_and_lengths(cuda):
    B, npoints = 4, 1024
    sweeps, lengths, Td = _case(B, regimes=False)
    dsweeps, dlen, dTd = sweeps.to(cuda), lengths.to(cuda), torch.from_numpy(Td).to(cuda)
    grab = lambda bld, out: [t.clone() for t in out] + [bld.indices().clone(), bld.aug_params().clone(), bld.t_gt().clone()]
    same = lambda u, v: all(torch.equal(a, b) for a, b in zip(u, v))

    eager = _builder("kitti360", B, npoints, 40000, seed=9)
    want = [grab(eager, eager.build(dsweeps, dlen, dTd)) for _ in range(3)]
    assert eager.step_index() == 3 and not same(want[0], want[1]) and not same(want[1], want[2])
    eager.set_step(40)
    want40 = grab(eager, eager.build(dsweeps, dlen, dTd))

    twin = _builder("kitti360", B, npoints, 40000, seed=9)                      # same seed: same batches
    assert same(grab(twin, twin.build(dsweeps, dlen, dTd)), want[0])
    other = _builder("kitti360", B, npoints, 40000, seed=10)
    assert not same(grab(other, other.build(dsweeps, dlen, dTd)), want[0])

    graphed = _builder("kitti360", B, npoints, 40000, seed=9)
    graphed.build(dsweeps, dlen, dTd)                                           # buffers and one-time attributes, eagerly
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = graphed.build(dsweeps, dlen, dTd)
    graphed.set_step(0)
    for k in range(3):
        g.replay()
        assert same(grab(graphed, out), want[k]), k                             # eager step k == replay at step k
    assert graphed.step_index() == 3
    graphed.set_step(40)
    g.replay()
    assert same(grab(graphed, out), want40)

    # the same capture with other lengths (device memory is read at replay)
    short = (lengths // 2).clamp(min=1)
    dlen.copy_(short)
    graphed.set_step(1)
    g.replay()
    torch.cuda.synchronize()
    ref = model.build("kitti360", sweeps.numpy(), short.numpy(), Td, npoints, 9, 1)
    assert np.array_equal(graphed.indices().cpu().numpy(), ref["indices"])
    assert np.array_equal(graphed.survivor_counts().cpu().numpy(), ref["counts"])


def test_builder_graph_in_front_of_a_graphed_train_step(cuda):
    """``out=``: the builder writes the static tensors a graphed TrainStep was captured on; builder replay + step replay
    gives the loss bits of an eager TrainStep fed clones of the same three batches."""
    from oracle import params
    from pwclonet_pylidarslam_amd.loss import PWCLONetLossModule
    from pwclonet_pylidarslam_amd.pointnet2_ops import pointnet2_utils
    from pwclonet_pylidarslam_amd.pwclonet import PWCLONet
    from pwclonet_pylidarslam_amd.training import PWCLONetWithLoss, TrainStep, set_reference_train_mode

    B, npoints = 2, 1024
    sweeps, lengths, Td = _case(B, regimes=False)
    dsweeps, dlen, dTd = sweeps.to(cuda), lengths.to(cuda), torch.from_numpy(Td).to(cuda)
    pointnet2_utils.deterministic_grads(True)             # atomics-free scatter-adds: run-to-run identical gradients
    try:
        net = PWCLONet(dict(num_input_channels=3, sequence_len=2, device=str(cuda), scalar_last=False, log_mode="none",
                            fused="off"))
        params.fill_state_dict(net.state_dict())
        net = set_reference_train_mode(net.to(cuda), dropout=False)
        loss_cfg = dict(with_exp_weights=True, init_weights=[0.0, -2.5], loss_option="l2_norm", nb_levels=4, scalar_last=False)
        unit = PWCLONetWithLoss(net, PWCLONetLossModule(loss_cfg).to(cuda))
        init = {k: v.detach().clone() for k, v in unit.state_dict().items()}

        def fresh(opt):                                   # the weights and Adam's state as before any step
            unit.load_state_dict(init)
            for st in opt.state.values():
                for v in st.values():
                    if isinstance(v, torch.Tensor):
                        v.zero_()

        # the three batches, eagerly, kept as clones
        bld = _builder("kitti360", B, npoints, 40000, seed=31)
        batches = [tuple(t.clone() for t in bld.build(dsweeps, dlen, dTd)) for _ in range(3)]
        assert not torch.equal(batches[0][0], batches[1][0])

        opt = torch.optim.Adam(unit.parameters(), lr=1e-3, capturable=True, fused=True)
        args = tuple(t.clone() for t in batches[0])
        ts = TrainStep(unit, opt, *args, graph=False)
        ts.step()                                         # creates Adam's state
        fresh(opt)
        eager = []
        for k in range(3):
            for dst, src in zip(args, batches[k]):
                dst.copy_(src)
            eager.append(ts.step().detach().clone())
        torch.cuda.synchronize()

        static = tuple(t.clone() for t in batches[0])
        opt = torch.optim.Adam(unit.parameters(), lr=1e-3, capturable=True, fused=True)
        unit.load_state_dict(init)
        ts = TrainStep(unit, opt, *static, graph=True, warmup=1)
        bld.set_step(0)
        bg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(bg):
            bld.build(dsweeps, dlen, dTd, out=static)
        fresh(opt)
        bld.set_step(0)
        graphed = []
        for k in range(3):
            bg.replay()
            assert all(torch.equal(a, b) for a, b in zip(static, batches[k])), k
            graphed.append(ts.step().detach().clone())
        torch.cuda.synchronize()
        for k in range(3):
            print("step %d: loss eager %.9g graphed %.9g" % (k, eager[k].item(), graphed[k].item()))
        assert all(torch.isfinite(v) for v in eager) and eager[0].item() != eager[1].item()
        for k in range(3):
            assert torch.equal(eager[k], graphed[k]), (k, eager[k].item(), graphed[k].item())
    finally:
        pointnet2_utils._DETERMINISTIC = None
