"""The flat data-parallel step on the GPU (run with ``-m gpu``): csrc/flat_step.hip's pack and Adam kernels on a synthetic
tensor list, ``flat_step.FlatAdam``'s device learning rate, skip on non-finite gradients and checkpoint round trip with
``torch.optim.Adam``, and ``FlatTrainStep`` on the whole training unit, eager, as graphs and over a world-size-1 RCCL group.

Adam criterion.  Truth is torch's own optimizer on float64 copies (``foreach=False``); the yardstick is torch's own fp32
optimizer on the same inputs, computed here.  Parameter errors are taken in units of ``lr``, moment errors in units of
``max|moment|``; over all values of all tensors this path's error must be <= 4 x the yardstick's maximum and <= 2 x its
rms (the factors tests/test_gpu_train.py uses for gradients).  The yardstick is 2e-4 ... 1.2e-3 ``lr`` at the maximum for the
synthetic inputs -- the rounding of a parameter of magnitude 2 ... 4 -- and a wrong bias correction or decay is O(1) ``lr``.
"""
import copy
import functools
import os

import pytest
import torch

from oracle import params as oracle_params
from pwclonet_pylidarslam_amd import _lib, synthetic
from pwclonet_pylidarslam_amd.flat_step import FlatAdam, FlatTrainStep, bucket_layout
from pwclonet_pylidarslam_amd.loss import PWCLONetLossModule
from pwclonet_pylidarslam_amd.pointnet2_ops import pointnet2_utils
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet
from pwclonet_pylidarslam_amd.training import PWCLONetWithLoss, set_reference_train_mode

pytestmark = pytest.mark.gpu
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
MAX_FACTOR, RMS_FACTOR = 4.0, 2.0
UNALIGNED = 8                      # index of the 4099-value tensor: allocated 4 bytes past a 16-byte boundary
CASES = [("adam", 0.0), ("adam", 1e-2), ("adamw", 1e-2)]


# ---- the synthetic tensor list ------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def _sizes():
    cap = _lib.load().flat_step_entries_per_launch()
    head = [1, 2, 3, 5, 64, 255, 256, 257, 4099, 70001]
    return tuple(head + [7] * (2 * cap + 1 - len(head)))          # longer than two launches' entry capacity


@functools.lru_cache(None)
def _inputs():
    """(parameters, gradients) on the host: parameters ~ N(0, 1), gradient magnitudes log-uniform over 1e-6 ... 10."""
    g = torch.Generator().manual_seed(1234)
    ps = [torch.randn(n, generator=g) for n in _sizes()]
    gs = [torch.pow(10.0, torch.rand(n, generator=g) * 7.0 - 6.0) * (torch.randint(0, 2, (n,), generator=g) * 2.0 - 1.0)
          for n in _sizes()]
    return ps, gs


def _to_device(ts, dev, leaf=False):
    out = []
    for i, t in enumerate(ts):
        if i == UNALIGNED:
            d = torch.empty(t.numel() + 1, device=dev)[1:]
            d.copy_(t)
            assert d.data_ptr() % 16 == 4
        else:
            d = t.to(dev)
        out.append(torch.nn.Parameter(d) if leaf else d)
    return out


def _flat(dev, kind="adam", wd=0.0, ps=None):
    ps = _to_device(_inputs()[0] if ps is None else ps, dev, leaf=True)
    gs = _to_device(_inputs()[1], dev)
    assert ps[UNALIGNED].data_ptr() % 16 == 4 and gs[UNALIGNED].data_ptr() % 16 == 4
    for p, g in zip(ps, gs):
        p.grad = g
    return FlatAdam(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, decoupled=kind == "adamw"), ps, gs


def _moments(opt, which):
    flat = getattr(opt, which)
    return [opt.view(flat, i) for i in range(len(opt.params))]


@functools.lru_cache(None)
def _torch_run(kind, wd, dtype, lr_after_first=None, steps=3):
    """torch's own Adam / AdamW on host copies of the synthetic list: (parameters, exp_avg, exp_avg_sq) after ``steps``."""
    P, G = _inputs()
    ps = [torch.nn.Parameter(p.to(dtype).clone()) for p in P]
    cls = torch.optim.AdamW if kind == "adamw" else torch.optim.Adam
    opt = cls(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, foreach=False)
    for k in range(steps):
        for p, g in zip(ps, G):
            p.grad = g.to(dtype).clone()
        opt.step()
        if k == 0 and lr_after_first is not None:
            for grp in opt.param_groups:
                grp["lr"] = lr_after_first
    return ([p.detach() for p in ps], [opt.state[p]["exp_avg"] for p in ps], [opt.state[p]["exp_avg_sq"] for p in ps])


def _err(got, ref64, unit):
    """(max, rms) over all values of all tensors of |got - ref64| / unit."""
    d = torch.cat([(a.detach().cpu().double().reshape(-1) - r.reshape(-1)).abs() for a, r in zip(got, ref64)]) / unit
    return d.max().item(), d.pow(2).mean().sqrt().item()


def _judge(what, got, yard, ref64, lr=LR):
    """got / yard / ref64: (parameters, exp_avg, exp_avg_sq) of this path, of torch's fp32 optimizer and of the float64 one."""
    for name, a, y, r in zip(("parameters [lr]", "exp_avg [max|m|]", "exp_avg_sq [max|v|]"), got, yard, ref64):
        unit = lr if name.startswith("parameters") else max(t.abs().max().item() for t in r)
        (emax, erms), (ymax, yrms) = _err(a, r, unit), _err(y, r, unit)
        print("\n%s, %s: this path max %.2e rms %.2e; torch fp32 max %.2e rms %.2e" % (what, name, emax, erms, ymax, yrms))
        assert emax <= MAX_FACTOR * ymax, (what, name, emax, ymax)
        assert erms <= RMS_FACTOR * yrms, (what, name, erms, yrms)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


# ---- pack ---------------------------------------------------------------------------------------------------------------

def test_pack_is_the_concatenation_bit_for_bit(cuda):
    opt, ps, gs = _flat(cuda)
    assert len(ps) > 2 * _lib.load().flat_step_entries_per_launch()
    offsets, total = bucket_layout(_sizes())
    assert (opt.offsets, opt.total) == (offsets, total)
    opt.bucket.fill_(123.0)                               # stale values everywhere: the padding must be WRITTEN as zero
    opt.pack(1.0)
    want = torch.zeros(total, device=cuda)
    for o, g in zip(offsets, gs):
        want[o:o + g.numel()] = g
    assert torch.equal(_bits(opt.bucket), _bits(want))    # values, zero padding and a zero count slot
    assert opt.nonfinite.item() == 0.0
    for i, g in enumerate(gs):
        assert torch.equal(_bits(opt.view(opt.bucket, i)), _bits(g)), i


def test_pack_scales_exactly(cuda):
    opt, ps, gs = _flat(cuda)
    opt.pack(1.0 / 8.0)
    for i, g in enumerate(gs):
        assert torch.equal(_bits(opt.view(opt.bucket, i)), _bits(g * 0.125)), i
    assert opt.nonfinite.item() == 0.0


def test_pack_counts_non_finite_values(cuda):
    opt, ps, gs = _flat(cuda)
    gs[5][17] = float("nan")
    gs[UNALIGNED][4098] = float("-inf")
    opt.pack(0.5)
    assert opt.nonfinite.item() == 2.0
    assert torch.isnan(opt.view(opt.bucket, 5)[17]) and opt.view(opt.bucket, UNALIGNED)[4098].item() == float("-inf")
    gs[5][17] = 1.0
    gs[UNALIGNED][4098] = 1.0
    opt.pack(0.5)                                         # the count starts from zero at every pack
    assert opt.nonfinite.item() == 0.0


def test_pack_refuses_what_it_cannot_gather(cuda):
    opt, ps, gs = _flat(cuda)
    ps[3].grad = None
    with pytest.raises(RuntimeError, match="no gradient"):
        opt.pack(1.0)
    with pytest.raises(RuntimeError, match="CPU not supported"):       # (torch itself refuses a host gradient on a device tensor)
        FlatAdam([torch.nn.Parameter(torch.zeros(5))], lr=LR)


# ---- Adam ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,wd", CASES)
def test_adam_three_steps_against_float64(cuda, kind, wd):
    opt, ps, gs = _flat(cuda, kind, wd)
    for _ in range(3):
        opt.pack(1.0)
        opt.step()
    assert opt.step_count.item() == 3
    got = (ps, _moments(opt, "exp_avg"), _moments(opt, "exp_avg_sq"))
    _judge("%s wd=%g, 3 steps" % (kind, wd), got, _torch_run(kind, wd, torch.float32), _torch_run(kind, wd, torch.float64))
    for flat in (opt.exp_avg, opt.exp_avg_sq):            # the moments' padding stays zero
        pad = torch.ones(opt.total, dtype=torch.bool, device=cuda)
        for o, n in zip(opt.offsets, opt.sizes):
            pad[o:o + n] = False
        assert not flat[pad].any()


def test_learning_rate_is_read_from_the_device(cuda):
    opt, ps, gs = _flat(cuda, "adam", 1e-2)
    for k in range(3):
        opt.pack(1.0)
        opt.step()
        if k == 0:
            opt.set_lr(5e-4)
    got = (ps, _moments(opt, "exp_avg"), _moments(opt, "exp_avg_sq"))
    _judge("adam wd=1e-2, lr 1e-3 then 5e-4", got, _torch_run("adam", 1e-2, torch.float32, 5e-4),
           _torch_run("adam", 1e-2, torch.float64, 5e-4), lr=5e-4)
    plain = _torch_run("adam", 1e-2, torch.float64)[0]    # ... and the schedule is not a no-op at this bound
    assert _err(ps, plain, 5e-4)[0] > 0.5


def test_step_is_skipped_on_non_finite_gradients(cuda):
    opt, ps, gs = _flat(cuda, "adam", 1e-2)
    clean, ref_ps, _ = _flat(cuda, "adam", 1e-2)          # the run that never sees the NaN
    opt.pack(1.0)
    opt.step()
    clean.pack(1.0)
    clean.step()
    keep = gs[7][100].item()
    gs[7][100] = float("nan")
    before = [_bits(t).clone() for t in ps + [opt.exp_avg, opt.exp_avg_sq, opt.step_count.view(torch.int32)]]
    opt.pack(1.0)
    opt.step()
    after = [_bits(t) for t in ps + [opt.exp_avg, opt.exp_avg_sq, opt.step_count.view(torch.int32)]]
    assert opt.nonfinite.item() == 1.0 and opt.step_count.item() == 1
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    gs[7][100] = keep
    opt.pack(1.0)
    opt.step()
    clean.pack(1.0)
    clean.step()
    assert opt.step_count.item() == 2 and opt.nonfinite.item() == 0.0
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(ps, ref_ps))
    assert torch.equal(_bits(opt.exp_avg), _bits(clean.exp_avg)) and torch.equal(_bits(opt.exp_avg_sq), _bits(clean.exp_avg_sq))


def test_checkpoint_round_trip_with_torch_adam(cuda):
    """torch.optim.Adam -> FlatAdam -> torch.optim.Adam through ``state_dict()`` / ``load_state_dict()``."""
    wd = 1e-2
    P, G = _inputs()
    tp = [torch.nn.Parameter(p.to(cuda)) for p in P]
    tg = [g.to(cuda) for g in G]
    topt = torch.optim.Adam(tp, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, fused=False)
    for _ in range(2):
        for p, g in zip(tp, tg):
            p.grad = g.clone()
        topt.step()
    sd = copy.deepcopy(topt.state_dict())                # (state_dict() hands out the live ``step`` tensors)
    opt, ps, gs = _flat(cuda, "adam", 0.0, ps=[p.detach().cpu() for p in tp])      # hyper-parameters come from the checkpoint
    opt.load_state_dict(sd)
    assert opt.step_count.item() == 2 and opt.weight_decay == wd and not opt.decoupled
    for i, p in enumerate(tp):
        assert torch.equal(opt.view(opt.exp_avg, i), topt.state[p]["exp_avg"])
        assert torch.equal(opt.view(opt.exp_avg_sq, i), topt.state[p]["exp_avg_sq"])
    # float64 truth of the third step from the same checkpoint
    dp = [torch.nn.Parameter(p.detach().cpu().double()) for p in tp]
    dopt = torch.optim.Adam(dp, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, foreach=False)
    dopt.load_state_dict(copy.deepcopy(sd))              # (torch casts the moments to the parameters' float64)
    for p, g in zip(dp, G):
        p.grad = g.double()
    dopt.step()
    for p, g in zip(tp, tg):
        p.grad = g.clone()
    topt.step()
    opt.pack(1.0)
    opt.step()
    assert opt.step_count.item() == 3
    truth = ([p.detach() for p in dp], [dopt.state[p]["exp_avg"] for p in dp], [dopt.state[p]["exp_avg_sq"] for p in dp])
    yard = (tp, [topt.state[p]["exp_avg"] for p in tp], [topt.state[p]["exp_avg_sq"] for p in tp])
    _judge("third step after loading torch's checkpoint", (ps, _moments(opt, "exp_avg"), _moments(opt, "exp_avg_sq")), yard,
           truth)
    ymax = _err(tp, truth[0], LR)[0]
    # ... and back: torch's optimizer loads FlatAdam's checkpoint and steps from it
    back = opt.state_dict()
    assert sorted(back) == ["param_groups", "state"] and sorted(back["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    bp = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    bopt = torch.optim.Adam(bp, lr=1.0, fused=False)
    bopt.load_state_dict(back)
    assert bopt.param_groups[0]["lr"] == LR and bopt.param_groups[0]["weight_decay"] == wd
    assert all(float(bopt.state[p]["step"]) == 3.0 for p in bp)
    for i, p in enumerate(bp):
        assert torch.equal(bopt.state[p]["exp_avg"], opt.view(opt.exp_avg, i))
    for p, g in zip(bp, tg):
        p.grad = g.clone()
    bopt.step()
    opt.pack(1.0)
    opt.step()
    # both took the fourth step from the same bits: they differ by at most the sum of two fp32 evaluations' errors, each
    # bounded as above by 4 x the yardstick
    diff = max((a.detach() - b.detach()).abs().max().item() for a, b in zip(bp, ps)) / LR
    print("fourth step, torch from FlatAdam's checkpoint vs FlatAdam: max difference %.2e lr (yardstick %.2e)" % (diff, ymax))
    assert 0.0 < max((a.detach() - p0.to(cuda)).abs().max().item() for a, p0 in zip(bp, P)) and diff <= 2 * MAX_FACTOR * ymax


# ---- the whole training unit --------------------------------------------------------------------------------------------

LOSS_CFG = dict(with_exp_weights=True, init_weights=[0.0, -2.5], loss_option="l2_norm", nb_levels=4, scalar_last=False)
_STATE = {}


@pytest.fixture
def deterministic():
    pointnet2_utils.deterministic_grads(True)      # atomics-free scatter-adds: run-to-run identical gradients
    yield
    pointnet2_utils._DETERMINISTIC = None


def _unit_and_batch(dev):
    """The training fixture's unit and batch, built once; every run starts from the same ``init`` state."""
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
        _STATE.update(unit=unit, batch=(x1, x2, gt), init={k: v.detach().clone() for k, v in unit.state_dict().items()},
                      runs={})
    return _STATE["unit"], _STATE["batch"], _STATE["init"]


def test_unit_bucket_holds_every_gradient_and_first_step(cuda, deterministic):
    unit, (x1, x2, gt), init = _unit_and_batch(cuda)
    unit.load_state_dict(init)
    unit.zero_grad(set_to_none=True)
    opt = FlatAdam(unit.parameters(), lr=LR, betas=BETAS, eps=EPS)
    names = [k for k, p in unit.named_parameters() if p.requires_grad]
    assert sum(opt.sizes) == 775070 and names[-1] == "loss_module.exp_weighting.s_param" and opt.sizes[-1] == 2
    loss, _, _ = unit(x1, x2, gt)
    loss.backward()
    opt.pack(1.0)
    for i, p in enumerate(opt.params):
        assert torch.equal(_bits(opt.view(opt.bucket, i)), _bits(p.grad)), names[i]
    assert opt.view(opt.bucket, len(names) - 1).abs().min().item() > 0.0          # the loss weights' gradients are in it
    assert opt.nonfinite.item() == 0.0
    grads = [opt.view(opt.bucket, i).detach().cpu() for i in range(len(names))]
    start = [p.detach().cpu() for p in opt.params]

    def torch_step(dtype):
        ps = [torch.nn.Parameter(p.to(dtype).clone()) for p in start]
        o = torch.optim.Adam(ps, lr=LR, betas=BETAS, eps=EPS, foreach=False)
        for p, g in zip(ps, grads):
            p.grad = g.to(dtype)
        o.step()
        return [p.detach() for p in ps], [o.state[p]["exp_avg"] for p in ps], [o.state[p]["exp_avg_sq"] for p in ps]

    opt.step()
    _judge("training unit, one step", (opt.params, _moments(opt, "exp_avg"), _moments(opt, "exp_avg_sq")),
           torch_step(torch.float32), torch_step(torch.float64))


def _run(dev, graph, group):
    """One warm-up step plus three steps from ``init``: (loss, parameters and buffers, exp_avg, exp_avg_sq, counter)."""
    key = (graph, group is not None)
    unit, batch, init = _unit_and_batch(dev)
    if key not in _STATE["runs"]:
        unit.load_state_dict(init)
        unit.zero_grad(set_to_none=True)
        opt = FlatAdam(unit.parameters(), lr=LR, betas=BETAS, eps=EPS, weight_decay=1e-2)
        ts = FlatTrainStep(unit, opt, *batch, graph=graph, process_group=group, warmup=1)
        if not graph:
            ts.step()                                   # the eager run takes its "warm-up" step by hand
        for _ in range(3):
            loss = ts.step()
        torch.cuda.synchronize()
        assert graph == (ts.front is not None) and (ts.back is not None) == (graph and group is not None)
        _STATE["runs"][key] = (loss.detach().clone(), {k: v.detach().clone() for k, v in unit.state_dict().items()},
                               opt.exp_avg.clone(), opt.exp_avg_sq.clone(), int(opt.step_count.item()),
                               float(opt.nonfinite.item()))
    return _STATE["runs"][key]


def _same_bits(a, b):
    assert torch.isfinite(a[0]) and torch.equal(_bits(a[0]), _bits(b[0])), (a[0].item(), b[0].item())
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    assert torch.equal(_bits(a[2]), _bits(b[2])) and torch.equal(_bits(a[3]), _bits(b[3]))
    assert a[4] == b[4] == 3 + 1 and a[5] == b[5] == 0.0        # three steps plus the one warm-up step


def test_flat_train_step_graph_equals_eager(cuda, deterministic):
    eager, graphed = _run(cuda, False, None), _run(cuda, True, None)
    _, _, init = _unit_and_batch(cuda)
    assert any((eager[1][k] != init[k]).any() for k in init if k.endswith("conv.weight"))       # the optimizer stepped
    _same_bits(eager, graphed)


def test_flat_train_step_world_size_1_nccl_equals_no_group(cuda, deterministic):
    import torch.distributed as dist
    plain = _run(cuda, True, None)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29641")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=cuda)
    try:
        grouped = _run(cuda, True, dist.group.WORLD)
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    _same_bits(plain, grouped)
