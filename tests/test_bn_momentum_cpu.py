"""CPU tests (``-m "not gpu"``) of the per-epoch schedules' host side: ``training.EpochSchedule``
drives any torch learning-rate scheduler class through its private optimizer and hands the optimizer the same rates that
class produces on a real ``torch.optim.Adam``, a checkpoint in the middle continues the sequence, ``BNMomentumScheduler``
without a cell is what it was, and the C ABI's ``_devmom`` siblings differ from the originals in the one argument.
"""
import ctypes
import warnings

import pytest
import torch
import torch.nn as nn
from torch.optim.lr_scheduler import CosineAnnealingLR, LRScheduler, MultiStepLR

from pwclonet_pylidarslam_amd import _lib
from pwclonet_pylidarslam_amd.pointnet2_ops import pytorch_utils as PT
from pwclonet_pylidarslam_amd.training import EpochSchedule

LR0, EPOCHS = 1e-3, 6


class FlooredExponential(LRScheduler):
    """lr(epoch) = max(lr0 * gamma ** epoch, floor), from the closed form."""

    def __init__(self, optimizer, gamma, floor):
        self.gamma, self.floor = gamma, floor
        super().__init__(optimizer)

    def get_lr(self):
        return [max(b * self.gamma ** self.last_epoch, self.floor) for b in self.base_lrs]


FACTORIES = {
    "multistep": lambda o: MultiStepLR(o, milestones=[1, 2, 4], gamma=0.5),
    "cosine": lambda o: CosineAnnealingLR(o, T_max=6, eta_min=1e-5),
    "floored_exponential": lambda o: FlooredExponential(o, gamma=0.5, floor=1e-4),
}


def _adam():
    return torch.optim.Adam([nn.Parameter(torch.zeros(3))], lr=LR0)


def _truth(name):
    """The rates the scheduler class gives a real Adam after each of EPOCHS epochs."""
    opt = _adam()
    sched = FACTORIES[name](opt)
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # (no optimizer.step() in between: torch's ordering warning)
        for _ in range(EPOCHS):
            sched.step()
            out.append(opt.param_groups[0]["lr"])
    return out


@pytest.mark.parametrize("name", sorted(FACTORIES))
def test_epoch_schedule_follows_the_scheduler_class(name):
    want = _truth(name)
    assert len(set(want)) > 2 and want[0] != LR0          # a schedule that moves
    opt = _adam()
    sch = EpochSchedule(opt, FACTORIES[name])
    got = []
    for _ in range(EPOCHS):
        sch.epoch_end()
        got.append(opt.param_groups[0]["lr"])
    assert got == want and sch.epoch == EPOCHS
    if name == "floored_exponential":
        assert want == [max(LR0 * 0.5 ** e, 1e-4) for e in range(1, EPOCHS + 1)] and want[-1] == 1e-4


def test_epoch_schedule_fills_a_tensor_learning_rate_in_place():
    opt = torch.optim.Adam([nn.Parameter(torch.zeros(3))], lr=torch.tensor(LR0))
    cell = opt.param_groups[0]["lr"]
    sch = EpochSchedule(opt, FACTORIES["multistep"])
    sch.epoch_end()
    assert opt.param_groups[0]["lr"] is cell and cell.item() == pytest.approx(LR0 * 0.5, rel=1e-7)


@pytest.mark.parametrize("name", sorted(FACTORIES))
def test_epoch_schedule_checkpoint_continues_the_sequence(name):
    want = _truth(name)
    opt = _adam()
    sch = EpochSchedule(opt, FACTORIES[name])
    for _ in range(3):
        sch.epoch_end()
    saved = sch.state_dict()
    opt2 = _adam()                                # a fresh process: the optimizer is at the initial rate again
    sch2 = EpochSchedule(opt2, FACTORIES[name])
    sch2.load_state_dict(saved)
    assert sch2.epoch == 3 and opt2.param_groups[0]["lr"] == want[2]         # loading pushed the rate
    got = []
    for _ in range(3):
        sch2.epoch_end()
        got.append(opt2.param_groups[0]["lr"])
    assert got == want[3:]


def _bn_model():
    return nn.Sequential(PT.Conv2d(3, 4, bn=True), PT.Conv1d(4, 5, bn=True), nn.BatchNorm3d(2))


def _ref_lambda(init=0.5, rate=0.5, step=1, top=0.99):
    return lambda it: min(1 - init * rate ** (int(it / step)), top)


def test_bn_scheduler_without_a_cell_is_unchanged():
    model = _bn_model()
    bns = [m for m in model.modules() if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d))]
    assert len(bns) == 3
    keys = list(model.state_dict())
    sched = PT.BNMomentumScheduler(model, _ref_lambda())
    assert sched.last_epoch == -1 and sched.last_momentum == 0.5 and all(m.momentum == 0.5 for m in bns)
    for epoch, want in ((1, 0.75), (2, 0.875), (7, 0.99)):
        sched.step(epoch)
        assert sched.last_epoch == epoch and sched.last_momentum == want and all(m.momentum == want for m in bns)
    sched.step()
    assert sched.last_epoch == 8
    assert not any("_pwclo_bn_momentum" in m.__dict__ for m in model.modules()) and list(model.state_dict()) == keys


def test_cell_on_a_cpu_model_follows_the_scheduler_and_detaches():
    """The cell's host side needs no GPU: attach, schedule, epoch schedule, guards at attach, detach."""
    model = _bn_model()
    keys = list(model.state_dict())
    cell = PT.attach_bn_momentum(model)
    assert isinstance(cell, PT.BNMomentumCell) and cell.value == 0.1 and cell.tensor.dtype == torch.float32
    assert cell.tensor.shape == (1,) and len(cell.modules) == 3 and list(model.state_dict()) == keys
    assert not any(t is cell.tensor for t in list(model.buffers()) + list(model.parameters()))
    with pytest.raises(RuntimeError, match="already"):
        PT.attach_bn_momentum(model)
    bn_sched = PT.BNMomentumScheduler(model, _ref_lambda())
    assert cell.value == 0.5 and cell.tensor.item() == 0.5
    sch = EpochSchedule(_adam(), None, bn_sched)
    sch.epoch_end()
    assert cell.value == 0.75 and cell.tensor.item() == 0.75 and all(m.momentum == 0.75 for m in cell.modules)
    cell.set(0.3)
    assert cell.tensor.item() == torch.tensor(0.3, dtype=torch.float32).item() and model[2].momentum == 0.3
    sch.load_state_dict({"epoch": 2, "lr_scheduler": None})
    assert cell.value == 0.875 and cell.tensor.item() == 0.875
    x = torch.randn(2, 2, 3, 3, 3)
    model[2](x)                                    # torch's own forward outside a capture: runs as ever
    cell.detach()
    assert not any("_pwclo_bn_momentum" in m.__dict__ for m in model.modules()) and list(model.state_dict()) == keys
    assert not model[2]._forward_pre_hooks
    bn_sched.step(1)                               # ... and the scheduler is the reference's again
    assert all(m.momentum == 0.75 for m in cell.modules) and cell.value == 0.875


def test_attach_refuses_differing_momenta():
    model = _bn_model()
    model[2].momentum = 0.2
    with pytest.raises(ValueError, match="ONE value"):
        PT.attach_bn_momentum(model)
    model[2].momentum = None
    with pytest.raises(ValueError, match="ONE value"):
        PT.attach_bn_momentum(model)
    with pytest.raises(ValueError, match="no BatchNorm"):
        PT.attach_bn_momentum(nn.Linear(2, 2))


def test_devmom_signatures_differ_in_the_momentum_argument_only():
    for name in ("batchnorm_train_forward_kernel_wrapper", "batchnorm_train_relu_maxk_forward_kernel_wrapper",
                 "conv1x1_forward_bnstats_kernel_wrapper"):
        sibling = name.replace("_kernel_wrapper", "_devmom_kernel_wrapper")
        (args, res), (dargs, dres) = _lib.SIGNATURES[name], _lib.SIGNATURES[sibling]
        assert res is None and dres is None and len(args) == len(dargs)
        diff = [i for i, (a, d) in enumerate(zip(args, dargs)) if a is not d]
        assert len(diff) == 1, (name, diff)
        i = diff[0]
        assert args[i] is ctypes.c_float and dargs[i] is ctypes.c_void_p
        assert args[i - 1] is ctypes.c_float and dargs[i - 1] is ctypes.c_float        # eps stays in front of it
    a, s = _lib.SIGNATURES["flat_adam_kernel_wrapper"], _lib.SIGNATURES["flat_adam_skipped_kernel_wrapper"]
    assert s[0][:-1] == a[0] and s[0][-1] is ctypes.c_void_p
