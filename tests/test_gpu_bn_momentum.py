"""BatchNorm momentum from device memory on the GPU (run with ``-m gpu``): the ``_devmom`` entry
points of csrc/batchnorm.hip / csrc/conv1x1.hip against the launch-argument originals bit for bit and against float64, a
captured graph that follows ``BNMomentumCell.set``, the whole training unit under ``training.EpochSchedule`` -- graphs
against eager, ``FlatTrainStep`` and ``TrainStep`` -- the guards at the call sites, and ``FlatAdam.skipped``.

One case differs from the list it was written from: ``conv1x1_stats`` was asked for on x (2, 19, 50, 1), but the
convolution launchers refuse rows whose length is no multiple of 4 (csrc/conv1x1.hip ``conv_args_ok``), with or without a
cell; the case runs on (2, 19, 52, 1) -- still 19 -> 21 channels (six finish workgroups, the last one a quarter full) and
rows that fill no whole 32-pixel tile.
"""
import copy
import functools

import pytest
import torch
import torch.nn as nn
from torch.optim.lr_scheduler import MultiStepLR

from oracle import params as oracle_params
from pwclonet_pylidarslam_amd import _lib, batchnorm as hip_bn, conv1x1 as hip_conv, synthetic
from pwclonet_pylidarslam_amd.flat_step import FlatAdam, FlatTrainStep
from pwclonet_pylidarslam_amd.loss import PWCLONetLossModule
from pwclonet_pylidarslam_amd.pointnet2_ops import pointnet2_utils, pytorch_utils as PT
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet
from pwclonet_pylidarslam_amd.training import EpochSchedule, PWCLONetWithLoss, TrainStep, set_reference_train_mode

pytestmark = pytest.mark.gpu
MOMENTA = (0.5, 0.75, 0.99)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), what


def _bn(c, ndim, dev, seed=0):
    """A training-mode BatchNorm with uneven affine parameters and running statistics."""
    cls = {3: nn.BatchNorm1d, 4: nn.BatchNorm2d, 5: nn.BatchNorm3d}[ndim]
    bn = cls(c).train()
    g = torch.Generator().manual_seed(100 + seed + c)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(c, generator=g))
        bn.running_var.copy_(torch.rand(c, generator=g) + 0.5)
        bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=g) * 0.3)
    return bn.to(dev)


def _x(shape, dev, seed=0):
    g = torch.Generator().manual_seed(sum(shape) + seed)
    return (torch.randn(*shape, generator=g) * 1.7 + 0.6).to(dev)


class _Bag(nn.Module):
    """The modules of one case under one root, so that one cell covers them."""

    def __init__(self, *mods):
        super().__init__()
        self.mods = nn.ModuleList(mods)


def _sweep(call, bns, start, with_cell):
    """``call()`` twice in a row for every momentum of MOMENTA, each time from the statistics ``start``; through the
    float launch argument (``with_cell=False``) or an attached cell.  -> the list of everything each call produced."""
    bag = _Bag(*bns)
    cell = PT.attach_bn_momentum(bag) if with_cell else None
    out = []
    try:
        for m in MOMENTA:
            with torch.no_grad():
                for bn, (rm, rv, nbt) in zip(bns, start):
                    bn.running_mean.copy_(rm), bn.running_var.copy_(rv), bn.num_batches_tracked.copy_(nbt)
            if with_cell:
                cell.set(m)
                assert cell.value == m and all(bn.momentum == m for bn in bns)
            else:
                for bn in bns:
                    bn.momentum = m
            for _ in range(2):
                got = [t.detach().clone() for t in call()]
                for bn in bns:
                    got += [bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone()]
                out.append(got)
    finally:
        if cell is not None:
            cell.detach()
    torch.cuda.synchronize()
    return out


def _assert_sweeps_equal(call, bns, n_outputs):
    start = [(bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone()) for bn in bns]
    plain, celled = _sweep(call, bns, start, False), _sweep(call, bns, start, True)
    assert len(plain) == len(celled) == 2 * len(MOMENTA)
    for k, (a, b) in enumerate(zip(plain, celled)):
        assert len(a) == len(b) == n_outputs + 3 * len(bns)
        for i, (ta, tb) in enumerate(zip(a, b)):
            if ta.dtype == torch.int64:
                assert torch.equal(ta, tb), (k, i)
            else:
                _same(ta, tb, (k, i))
    # the sweep moved the statistics, and differently for every momentum: equal bits are not two no-ops
    first = [plain[2 * j][n_outputs] for j in range(len(MOMENTA))]
    assert not torch.equal(first[0], first[1]) and not torch.equal(first[1], first[2])
    assert not torch.equal(plain[0][n_outputs], plain[1][n_outputs])


def _saved_stats(y):
    """(save_mean, save_invstd) the training kernels left for the backward of ``y``."""
    saved = y.grad_fn.saved_tensors
    return saved[3], saved[4]


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", [(2, 5, 7), (3, 130, 4, 9)])
def test_batch_norm_train_sibling_equals_original(cuda, shape, relu):
    bn, x = _bn(shape[1], len(shape), cuda), _x(shape, cuda)

    def call():
        y = hip_bn.batch_norm_train(x, bn, relu=relu)
        return (y,) + _saved_stats(y)

    _assert_sweeps_equal(call, [bn], 3)


@pytest.mark.parametrize("k", [4, 8, 16, 32])
def test_batch_norm_train_relu_max_sibling_equals_original(cuda, k):
    shape = (2, 6, 33, k)
    bn, x = _bn(6, 4, cuda), _x(shape, cuda)
    assert hip_bn.supported_maxk(x, bn)

    def call():
        y = hip_bn.batch_norm_train_relu_max(x, bn)
        return (y,) + _saved_stats(y)

    _assert_sweeps_equal(call, [bn], 3)


def _conv(cin, cout, dev, seed):
    conv = nn.Conv2d(cin, cout, 1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=torch.Generator().manual_seed(seed)) * 0.3)
    return conv.to(dev)


def test_conv1x1_stats_sibling_equals_original(cuda):
    x = _x((2, 19, 52, 1), cuda)                  # (see the module docstring for 52)
    conv, bn = _conv(19, 21, cuda, 1), _bn(21, 4, cuda)
    assert hip_conv.supported(x, conv)

    def call():
        y, (mean, invstd) = hip_conv.conv1x1_stats(x, conv, bn)
        return y, mean, invstd

    _assert_sweeps_equal(call, [bn], 3)


def test_bn_relu_conv_chain_sibling_equals_original(cuda):
    """Two ``bn_relu_conv`` layers with ``next_bn``: the first takes its own statistics pass (the statistics-only call of
    ``_BNReluConv``), the second gets them from the first's epilogue; three BatchNorm layers are updated."""
    x = _x((2, 19, 52, 1), cuda)
    conv0, conv1, conv2 = _conv(19, 21, cuda, 1), _conv(21, 10, cuda, 2), _conv(10, 7, cuda, 3)
    bn0, bn1, bn2 = _bn(21, 4, cuda, 1), _bn(10, 4, cuda, 2), _bn(7, 4, cuda, 3)

    def call():
        y0 = hip_conv.conv1x1(x, conv0.weight)
        y1, s1 = hip_conv.bn_relu_conv(y0, bn0, conv1, next_bn=bn1)
        y2, s2 = hip_conv.bn_relu_conv(y1, bn1, conv2, stats=s1, next_bn=bn2)
        return (y1, y2, s1[0], s1[1], s2[0], s2[1]) + _saved_stats(y1)

    _assert_sweeps_equal(call, [bn0, bn1, bn2], 8)


def test_cell_values_against_float64(cuda):
    """(3, 130, 4, 9) through a cell, momentum 0.5 then 0.875, against ``F.batch_norm`` in float64 on the CPU; the bound
    is the one tests/test_gpu_ops.py puts on the running statistics (1e-6, relative to max(1, max|reference|)) and on
    the output (2e-6)."""
    shape = (3, 130, 4, 9)
    bn, x = _bn(130, 4, cuda), _x(shape, cuda)
    rm, rv = bn.running_mean.cpu().double(), bn.running_var.cpu().double()
    w, b = bn.weight.detach().cpu().double(), bn.bias.detach().cpu().double()
    cell = PT.attach_bn_momentum(_Bag(bn))

    def close(a, ref, tol):
        err = (a.detach().cpu().double() - ref).abs().max().item()
        print("max error %.3g (bound %.3g)" % (err, tol * max(1.0, ref.abs().max().item())))
        assert err <= tol * max(1.0, ref.abs().max().item()), err

    for m in (0.5, 0.875):
        cell.set(m)
        before = rm.clone()
        yr = torch.nn.functional.batch_norm(x.cpu().double(), rm, rv, w, b, True, m, bn.eps)
        y = hip_bn.batch_norm_train(x, bn)
        close(y, yr, 2e-6)
        close(bn.running_mean, rm, 1e-6)
        close(bn.running_var, rv, 1e-6)
        assert (rm - before).abs().max().item() > 1e-2           # the update is far above the bound
    assert int(bn.num_batches_tracked) == 2
    cell.detach()


def _replayed(cuda, with_cell):
    """One ``batch_norm_train`` call captured at momentum 0.5, replayed, momentum changed to 0.25, replayed."""
    shape = (3, 130, 4, 9)
    bn, x = _bn(130, 4, cuda), _x(shape, cuda)
    bn.momentum = 0.5
    start = (bn.running_mean.clone(), bn.running_var.clone())
    cell = PT.attach_bn_momentum(_Bag(bn)) if with_cell else None
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side), torch.no_grad():
        hip_bn.batch_norm_train(x, bn)              # allocator warm-up outside the capture
    torch.cuda.current_stream(cuda).wait_stream(side)
    torch.cuda.synchronize(cuda)
    with torch.no_grad():
        bn.running_mean.copy_(start[0]), bn.running_var.copy_(start[1])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        hip_bn.batch_norm_train(x, bn)
    graph.replay()
    if with_cell:
        cell.set(0.25)
    else:
        bn.momentum = 0.25
    graph.replay()
    torch.cuda.synchronize(cuda)
    if cell is not None:
        cell.detach()
    return bn.running_mean.clone(), bn.running_var.clone()


def test_replay_follows_the_cell(cuda):
    shape = (3, 130, 4, 9)
    bn, x = _bn(130, 4, cuda), _x(shape, cuda)
    with torch.no_grad():
        for m in (0.5, 0.25):
            bn.momentum = m
            hip_bn.batch_norm_train(x, bn)
    celled, plain = _replayed(cuda, True), _replayed(cuda, False)
    _same(celled[0], bn.running_mean, "running_mean")
    _same(celled[1], bn.running_var, "running_var")
    # the gap the cell closes: without it the second replay still blends with the capture's 0.5
    assert not torch.equal(plain[0], bn.running_mean) and not torch.equal(plain[1], bn.running_var)


# ---- guards ---------------------------------------------------------------------------------------------------------------

def _small_model(dev):
    torch.manual_seed(5)
    return nn.Sequential(PT.SharedMLP([6, 8, 12], bn=True), PT.Conv2d(12, 5, bn=True)).to(dev).train()


def test_momentum_assigned_behind_the_cell_is_refused(cuda):
    model, x = _small_model(cuda), _x((2, 6, 8, 4), cuda)
    cell = PT.attach_bn_momentum(model)
    model(x)
    model[1].bn.bn.momentum = 0.3
    with pytest.raises(RuntimeError, match="behind the attached cell"):
        model(x)
    model[1].bn.bn.momentum = cell.value
    model[0].layer1.bn.bn.momentum = 0.3            # an interior layer of the stack (conv1x1 call sites)
    with pytest.raises(RuntimeError, match="behind the attached cell"):
        model(x)
    cell.set(0.3)
    model(x)
    bn, xb = _bn(5, 3, cuda), _x((2, 5, 7), cuda)
    cell2 = PT.attach_bn_momentum(_Bag(bn))
    bn.momentum = 0.3
    with pytest.raises(RuntimeError, match="behind the attached cell"):
        hip_bn.batch_norm_train(xb, bn)
    cell2.detach()


def test_cell_on_another_device_is_refused(cuda):
    model = _small_model(torch.device("cpu"))
    cell = PT.attach_bn_momentum(model)             # the cell is made where the model is: on the host
    assert cell.tensor.device.type == "cpu"
    model.to(cuda)
    with pytest.raises(RuntimeError, match="lives on cpu"):
        model(_x((2, 6, 8, 4), cuda))


def test_differing_momenta_are_refused_at_attach(cuda):
    model = _small_model(cuda)
    model[1].bn.bn.momentum = 0.2
    with pytest.raises(ValueError, match="ONE value"):
        PT.attach_bn_momentum(model)


def test_detach_restores_a_model_that_never_had_a_cell(cuda):
    model, x = _small_model(cuda), _x((2, 6, 8, 4), cuda)
    never = copy.deepcopy(model)
    cell = PT.attach_bn_momentum(model)
    cell.set(0.4)
    model(x)
    cell.detach()
    for m in never.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.momentum = 0.4
    never(x)
    assert list(model.state_dict()) == list(never.state_dict())
    assert not any(hip_bn.CELL_ATTR in m.__dict__ for m in model.modules())
    for m in model.modules():                       # no cell: assigning the attribute is today's way again
        if isinstance(m, nn.BatchNorm2d):
            m.momentum = 0.2
            assert not m._forward_pre_hooks
    for m in never.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.momentum = 0.2
    _same(model(x), never(x), "forward after detach")
    for (k, a), b in zip(model.state_dict().items(), never.state_dict().values()):
        assert torch.equal(a, b), k


def test_torch_fallback_is_refused_only_inside_a_capture(cuda, monkeypatch):
    """A (B, C) input is a shape ``supported()`` rejects: the wrapper runs torch's ``batch_norm``, which takes the
    momentum as a host float.  Outside a capture that is today's behaviour; inside one it raises.  (The capture is
    stood in for by its query: the guard asks ``torch.cuda.is_current_stream_capturing``.)"""
    wrapped = PT.BatchNorm1d(5).to(cuda).train()
    never = copy.deepcopy(wrapped)
    x = _x((4, 5), cuda)
    cell = PT.attach_bn_momentum(wrapped)
    _same(wrapped(x), never(x), "torch path outside a capture")
    _same(wrapped.bn.running_var, never.bn.running_var, "running_var")
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="inside a graph capture"):
        wrapped(x)
    wrapped.eval()(x)                               # eval mode reads no momentum
    cell.detach()
    wrapped.train()(x)


# ---- the whole training unit ----------------------------------------------------------------------------------------------

LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
LOSS_CFG = dict(with_exp_weights=True, init_weights=[0.0, -2.5], loss_option="l2_norm", nb_levels=4, scalar_last=False)
_STATE = {}


@pytest.fixture
def deterministic():
    pointnet2_utils.deterministic_grads(True)      # atomics-free scatter-adds: run-to-run identical gradients
    yield
    pointnet2_utils._DETERMINISTIC = None


def _unit_and_batch(dev):
    if not _STATE:
        net = PWCLONet(dict(num_input_channels=3, sequence_len=2, device=str(dev), scalar_last=False, log_mode="none",
                            fused="off"))
        oracle_params.fill_state_dict(net.state_dict())
        net = set_reference_train_mode(net.to(dev), dropout=False)
        unit = PWCLONetWithLoss(net, PWCLONetLossModule(dict(LOSS_CFG)).to(dev))
        pc1, pc2 = synthetic.uniform_pair(77, 1024, 2)
        x1 = torch.from_numpy(pc1[:, :, :3]).permute(0, 2, 1).contiguous().to(dev)
        x2 = torch.from_numpy(pc2[:, :, :3]).permute(0, 2, 1).contiguous().to(dev)
        gt = torch.tensor([[0.1, 0.0, 0.5, 1.0, 0.0, 0.0, 0.0], [0.0, 0.1, 0.7, 0.999, 0.0, 0.04, 0.0]], device=dev)
        _STATE.update(unit=unit, batch=(x1, x2, gt), init={k: v.detach().clone() for k, v in unit.state_dict().items()})
    return _STATE["unit"], _STATE["batch"], _STATE["init"]


def _epochs(dev, flat, graph):
    """One warm-up step, then two epochs of two steps with ``epoch_end()`` between them, from ``init``, with a cell, the
    reference's momentum lambda (init 0.5, rate 0.5, step 1, max 0.99) and ``MultiStepLR(milestones=[1], gamma=0.5)``.
    -> (loss, unit state, exp_avg list, exp_avg_sq list, step counter, momentum and rate at the end)."""
    unit, batch, init = _unit_and_batch(dev)
    unit.load_state_dict(init)
    unit.zero_grad(set_to_none=True)
    cell = PT.attach_bn_momentum(unit)
    try:
        bn_sched = PT.BNMomentumScheduler(unit, lambda it: min(1 - 0.5 * 0.5 ** (int(it / 1)), 0.99))
        assert cell.value == 0.5
        if flat:
            opt = FlatAdam(unit.parameters(), lr=LR, betas=BETAS, eps=EPS)
        else:
            opt = torch.optim.Adam(unit.parameters(), lr=torch.tensor(LR, device=dev), betas=BETAS, eps=EPS, capturable=True)
        sch = EpochSchedule(opt, lambda o: MultiStepLR(o, milestones=[1], gamma=0.5), bn_sched)
        ts = (FlatTrainStep if flat else TrainStep)(unit, opt, *batch, graph=graph, warmup=1)
        if not graph:
            ts.step()                               # the eager run takes its "warm-up" step by hand
        for epoch in range(2):
            for _ in range(2):
                loss = ts.step()
            if epoch == 0:
                sch.epoch_end()
        torch.cuda.synchronize()
        assert cell.value == 0.75 and cell.tensor.item() == 0.75 and sch.epoch == 1
        if flat:
            assert graph == (ts.front is not None)
            moments = ([opt.exp_avg.clone()], [opt.exp_avg_sq.clone()])
            count, rate = int(opt.step_count.item()), float(opt.lr.item())
            assert opt.skipped.item() == 0
        else:
            assert graph == (ts.graph is not None)
            ps = [p for p in unit.parameters() if p.requires_grad]
            moments = ([opt.state[p]["exp_avg"].clone() for p in ps], [opt.state[p]["exp_avg_sq"].clone() for p in ps])
            count, rate = int(opt.state[ps[0]]["step"].item()), float(opt.param_groups[0]["lr"].item())
        assert count == 5 and rate == pytest.approx(LR * 0.5, rel=1e-6)
        return (loss.detach().clone(), {k: v.detach().clone() for k, v in unit.state_dict().items()}, moments[0],
                moments[1], count)
    finally:
        cell.detach()


def _same_runs(a, b):
    assert torch.isfinite(a[0]) and torch.equal(_bits(a[0]), _bits(b[0])), (a[0].item(), b[0].item())
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    for i in (2, 3):
        assert len(a[i]) == len(b[i]) and all(torch.equal(_bits(s), _bits(t)) for s, t in zip(a[i], b[i]))
    assert a[4] == b[4]


@pytest.mark.parametrize("flat", [True, False], ids=["FlatTrainStep", "TrainStep"])
def test_epochs_of_replays_equal_eager_epochs(cuda, deterministic, flat):
    """Fails without the cell: the graphed run keeps blending the running statistics with the capture's momentum 0.5
    through the second epoch, the eager run moves to 0.75."""
    eager, graphed = _epochs(cuda, flat, False), _epochs(cuda, flat, True)
    _, _, init = _unit_and_batch(cuda)
    moved = [k for k in init if k.endswith("running_mean") and (eager[1][k] != init[k]).any()]
    assert moved and any((eager[1][k] != init[k]).any() for k in init if k.endswith("conv.weight"))
    _same_runs(eager, graphed)


# ---- FlatAdam.skipped -----------------------------------------------------------------------------------------------------

UNALIGNED = 8                      # index of the 4099-value tensor: allocated 4 bytes past a 16-byte boundary


@functools.lru_cache(None)
def _sizes():
    cap = _lib.load().flat_step_entries_per_launch()
    head = [1, 2, 3, 5, 64, 255, 256, 257, 4099, 70001]
    return tuple(head + [7] * (2 * cap + 1 - len(head)))          # longer than two launches' entry capacity


def _flat(dev):
    g = torch.Generator().manual_seed(1234)
    host_p = [torch.randn(n, generator=g) for n in _sizes()]
    host_g = [torch.pow(10.0, torch.rand(n, generator=g) * 7.0 - 6.0) * (torch.randint(0, 2, (n,), generator=g) * 2.0 - 1.0)
              for n in _sizes()]

    def put(ts, leaf):
        out = []
        for i, t in enumerate(ts):
            if i == UNALIGNED:
                d = torch.empty(t.numel() + 1, device=dev)[1:]
                d.copy_(t)
            else:
                d = t.to(dev)
            out.append(nn.Parameter(d) if leaf else d)
        return out

    ps, gs = put(host_p, True), put(host_g, False)
    for p, gr in zip(ps, gs):
        p.grad = gr
    return FlatAdam(ps, lr=LR, betas=BETAS, eps=EPS), ps, gs


def test_skipped_steps_are_counted_across_packs_and_checkpoints(cuda):
    opt, ps, gs = _flat(cuda)
    assert len(ps) == 257 and opt.skipped.dtype == torch.int64 and opt.skipped.item() == 0
    for bad in (None, float("nan"), None, float("inf")):
        keep = gs[7][100].item()
        if bad is not None:
            gs[7][100] = bad
        opt.pack(1.0)
        opt.step()
        gs[7][100] = keep
    assert opt.skipped.item() == 2 and opt.step_count.item() == 2 and opt.nonfinite.item() == 1.0
    opt.pack(1.0)                                   # clean gradients: the bucket's count starts over, the total does not
    assert opt.nonfinite.item() == 0.0 and opt.skipped.item() == 2
    sd = opt.state_dict()
    assert sorted(sd) == ["param_groups", "state"] and sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    other, _, _ = _flat(cuda)
    other.load_state_dict(copy.deepcopy(sd))
    assert other.skipped.item() == 2 and other.step_count.item() == 2
    other.pack(1.0)
    other.step()
    assert other.skipped.item() == 2 and other.step_count.item() == 3
    old = copy.deepcopy(sd)
    del old["param_groups"][0]["flat_skipped"]      # a checkpoint of torch's own Adam, or of an earlier FlatAdam
    other.load_state_dict(old)
    assert other.skipped.item() == 0 and other.step_count.item() == 2
    topt = torch.optim.Adam([nn.Parameter(p.detach().clone()) for p in ps], lr=1.0, fused=False)
    topt.load_state_dict(sd)                        # torch's Adam carries the extra entry along and steps
    for p, gr in zip(topt.param_groups[0]["params"], gs):
        p.grad = gr.clone()
    topt.step()
    assert topt.param_groups[0]["lr"] == LR
