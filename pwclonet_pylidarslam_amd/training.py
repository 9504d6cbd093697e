"""The unit that data-parallel training replicates: network + loss in ONE module.

The reference's trainer optimises the prediction module's parameters together with the loss module's
learnable weights (``slam/training/trainer.py:268`` builds both; ``loss_modules.py:147-197``: the
``ExponentialWeights.s_param`` pair).  Under ``DistributedDataParallel`` every parameter the optimiser
steps must take part in the gradient all-reduce, otherwise each rank -- which sees different frame pairs --
drifts to its own loss weights and then to its own network.  ``PWCLONetWithLoss`` owns both, so that
``ddp(PWCLONetWithLoss(net, loss))`` reduces the 775 068 network gradients AND the 2 loss-weight gradients
("775 068 + 2 fp32 values = 3.10 MB per step") in one bucket.
"""
import torch
import torch.nn as nn

from . import _lib
from .flat_step import FlatAdam, FlatTrainStep  # noqa: F401  (the data-parallel step that replays as graphs)


class PWCLONetWithLoss(nn.Module):
    """``forward(xyz_f1 (B,3,N), xyz_f2 (B,3,N), gt_params (B,7)) -> (loss, pose_params (B,4,7), log_dict)``."""

    def __init__(self, net, loss_module):
        super().__init__()
        self.pwclonet = net
        self.loss_module = loss_module

    def forward(self, xyz_f1, xyz_f2, gt_params, samples=None):
        if samples is None:
            pose, _ = self.pwclonet(xyz_f1, None, xyz_f2, None)
        else:
            pose, _ = self.pwclonet(xyz_f1, None, xyz_f2, None, samples=samples)
        loss, log = self.loss_module(pose, gt_params)
        return loss, pose, log


def ddp_wrap(model, device=None, process_group=None):
    """``DistributedDataParallel`` over RCCL with the settings SURVEY.md section 8e derives for this model:
    BN buffers are NOT broadcast (the reference has no cross-rank BN), every parameter receives a gradient
    (``find_unused_parameters=False``), and the whole 3.1 MB gradient set travels as one bucket (the step is
    latency-bound over xGMI: a single all-reduce, not DDP's default 1 MB first bucket + remainder)."""
    from torch.nn.parallel import DistributedDataParallel as DDP
    kw = dict(broadcast_buffers=False, find_unused_parameters=False, bucket_cap_mb=16, process_group=process_group)
    if device is not None and device.type == "cuda":
        kw["device_ids"] = [device.index if device.index is not None else torch.cuda.current_device()]
    ddp = DDP(model, **kw)
    return ddp


def gradient_bucket_values(model):
    """Number of fp32 values one step's all-reduce carries (parameters that require grad)."""
    return sum(p.numel() for p in model.parameters() if p.requires_grad)


def set_reference_train_mode(net, dropout=True):
    """``net.train()`` as the reference's trainer leaves the model (batch-statistic BatchNorm everywhere,
    P2/pytorch_utils.py:52-83).  ``dropout=False`` additionally puts the four ``PoseCalculator`` heads -- which
    hold no BatchNorm, only the two ``F.dropout`` calls of PW/pose_calculator.py:63-65 -- into ``eval()``: the mode
    the training parity fixtures are recorded in (a dropout stream is not reproducible across devices)."""
    net.train()
    if not dropout:
        heads = [m for m in net.modules() if type(m).__name__ == "PoseCalculator"]
        assert len(heads) == 4, len(heads)
        for m in heads:
            m.eval()
    return net


class TrainStep:
    """One training step of the data-parallel unit -- ``zero_grad -> forward -> loss -> backward -> optimizer.step``
    (slam/training/trainer.py:624-628) -- launched eagerly or replayed as ONE hipGraph (``graph=True``; single
    process only: DDP's bucketed all-reduce is not captured here).  ``step()`` returns the loss tensor (static under
    the graph: read it before the next replay).

    ``sample_ahead=True``: the furthest-point sampling of the four pyramid levels -- a function of the input
    coordinates only, the longest serial kernel chain of the step (one workgroup per cloud: 1.9 + up to 0.7 ms on a
    quarter of the chip) -- is drawn for the NEXT batch on a second stream WHILE the current batch's step runs, the way
    a data loader prefetches: ``step(next_batch=(xyz_f1, xyz_f2, gt))`` trains on the batch loaded last (the
    constructor's at first), samples ``next_batch`` beside it and makes it current; ``step()`` keeps the same batch.
    Every step still runs one sampling chain and one forward / backward / optimizer step; the values are those of the
    plain step (same samples, bit for bit; tests/test_gpu_train.py).  Under ``graph=True`` the sampler is a second
    hipGraph replayed on the side stream.  OPT-IN, and measured (tools/sample_ahead_probe.py, profiles/r03): the step
    graph without its sampler replays in 25.2 ms instead of 27.7, but on this runtime a graph replayed on the default
    stream does not overlap with work of another stream (25.2 + 2.6 = 27.7 ms again), the same graph replayed on a
    non-default stream takes 56 ms, and a forked branch inside ONE graph 61 ms; eager kernels of two streams do overlap
    (20 matmuls + the sampler: 19.3 ms against 18.3 + 2.6), but the eager step is host-bound.  So today this buys
    nothing on one GPU; it is the hook a loader-side sampler needs."""

    def __init__(self, model, optimizer, xyz_f1, xyz_f2, gt_params, graph=False, warmup=3, sample_ahead=False):
        self.model, self.opt = model, optimizer
        self.args = (xyz_f1, xyz_f2, gt_params)
        self.graph = self.sample_graph = None
        self.samples = self.next_samples = None
        dev = xyz_f1.device
        if sample_ahead:
            unit = model.module if hasattr(model, "module") else model
            self.net = unit.pwclonet
            self.side = torch.cuda.Stream(device=dev)
            self.next_args = tuple(t.clone() for t in self.args)
            self.samples = self.net.sample_pyramid(xyz_f1, xyz_f2)            # prologue: the first batch's own samples
            self.samples = tuple([t.clone() for t in lv] for lv in self.samples)
        if graph:
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(warmup):                 # allocator / autograd warm-up outside the capture
                    self._eager()
                    if sample_ahead:
                        self._sample_next()
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
            self.graph = torch.cuda.CUDAGraph()
            self.opt.zero_grad(set_to_none=True)
            with _lib.capture(self.graph):
                self.static_loss, _pose, _log = self._forward()
                self.static_loss.backward()
                self.opt.step()
            if sample_ahead:
                self.sample_graph = torch.cuda.CUDAGraph()
                with _lib.capture(self.sample_graph):
                    self._sample_next()
                torch.cuda.synchronize(dev)

    def _forward(self):
        if self.samples is None:
            return self.model(*self.args)
        return self.model(*self.args, samples=self.samples)

    def _sample_next(self):
        nxt = self.net.sample_pyramid(self.next_args[0], self.next_args[1])
        if self.next_samples is None:
            self.next_samples = tuple([t.clone() for t in lv] for lv in nxt)
        else:
            for dst, src in zip(self.next_samples, nxt):
                torch._foreach_copy_(dst, src)

    def _eager(self):
        self.opt.zero_grad(set_to_none=True)
        loss, _pose, _log = self._forward()
        loss.backward()
        self.opt.step()
        return loss

    def step(self, next_batch=None):
        if self.samples is None:
            if next_batch is not None:
                raise ValueError("next_batch needs TrainStep(sample_ahead=True); load a batch by copying into the tensors "
                                 "the step was built on")
            if self.graph is None:
                return self._eager()
            self.graph.replay()                         # gradients are overwritten in place by the replay
            return self.static_loss
        cur = torch.cuda.current_stream(self.args[0].device)
        if next_batch is not None:
            torch._foreach_copy_(list(self.next_args), list(next_batch))
        self.side.wait_stream(cur)
        with torch.cuda.stream(self.side):              # the next batch's samples, beside this batch's step
            if self.sample_graph is not None:
                self.sample_graph.replay()
            else:
                self._sample_next()
        if self.graph is None:
            loss = self._eager()
        else:
            self.graph.replay()
            loss = self.static_loss
        cur.wait_stream(self.side)
        if next_batch is not None:
            torch._foreach_copy_(list(self.args), list(self.next_args))
        for dst, src in zip(self.samples, self.next_samples):
            torch._foreach_copy_(dst, src)
        return loss


class EpochSchedule:
    """The reference trainer's two per-epoch schedules (slam/training/trainer.py:469-482) tied to the device values a
    captured step reads: the learning rate (``FlatAdam.lr`` / a tensor ``lr`` of a capturable torch optimizer) and the
    BatchNorm momentum (``pytorch_utils.attach_bn_momentum``), DESIGN.md section 17.

    ``lr_scheduler_factory(opt) -> LRScheduler`` is called with a private one-parameter ``torch.optim.SGD`` whose ``lr``
    is ``optimizer``'s current learning rate, so any torch scheduler class constructs and steps on it unchanged
    (``FlatAdam`` is not a ``torch.optim.Optimizer``).  ``bn_scheduler``: a ``pytorch_utils.BNMomentumScheduler``.

    ``epoch_end()`` steps the learning-rate scheduler and pushes ``get_last_lr()[0]`` into ``optimizer`` -- every
    group's ``lr`` of a torch optimizer, filled in place where it is a tensor -- then steps the BatchNorm scheduler with
    ``epoch``, the number of epochs finished: the epoch the value is used for.  (The reference passes the 0-based index
    of the epoch just finished, so its momentum trails its own lambda by one epoch; shift the lambda to reproduce that.)"""

    def __init__(self, optimizer, lr_scheduler_factory=None, bn_scheduler=None):
        self.opt, self.bn_scheduler = optimizer, bn_scheduler
        self.epoch = 0
        self.lr_scheduler = self._proxy = None
        if lr_scheduler_factory is not None:
            lr = optimizer._lr_host if isinstance(optimizer, FlatAdam) else float(optimizer.param_groups[0]["lr"])
            self._proxy = torch.optim.SGD([nn.Parameter(torch.zeros(1))], lr=lr)
            self.lr_scheduler = lr_scheduler_factory(self._proxy)

    def _push(self):
        if self.lr_scheduler is not None:
            lr = float(self.lr_scheduler.get_last_lr()[0])
            if isinstance(self.opt, FlatAdam):
                self.opt.set_lr(lr)
            else:
                for g in self.opt.param_groups:
                    if torch.is_tensor(g["lr"]):
                        g["lr"].fill_(lr)
                    else:
                        g["lr"] = lr

    def epoch_end(self):
        self.epoch += 1
        if self.lr_scheduler is not None:
            self._proxy.step()                   # (nothing to update; torch warns when a scheduler steps first)
            self.lr_scheduler.step()
            self._push()
        if self.bn_scheduler is not None:
            self.bn_scheduler.step(self.epoch)

    def state_dict(self):
        return {"epoch": self.epoch,
                "lr_scheduler": self.lr_scheduler.state_dict() if self.lr_scheduler is not None else None}

    def load_state_dict(self, sd):
        """Resume: the epoch and the learning-rate scheduler's state; both values go to the device again."""
        self.epoch = int(sd["epoch"])
        if self.lr_scheduler is not None:
            self.lr_scheduler.load_state_dict(sd["lr_scheduler"])
            self._proxy.param_groups[0]["lr"] = self.lr_scheduler.get_last_lr()[0]      # the recursive forms start from it
            self._push()
        if self.bn_scheduler is not None:
            self.bn_scheduler.step(self.epoch)


class DropoutStream:
    """Replayable dropout for the four pose heads: while attached, a training-mode
    ``PWCLONet.forward`` on the GPU advances the step counter with one launch and every ``PoseCalculator`` in ``train()``
    mode runs ``pose_head.pose_head_train`` -- the head as hand-written kernels -- with keep masks that are a function of
    ``(seed, step, rank, head, branch, cloud, unit)``: Philox4x32-10 under the 64-bit ``seed``, the generator of
    ``batches.TrainBatchBuilder`` with purpose word 3.  The reference's ``F.dropout`` stream is not reproduced, its law is
    (p = 0.5: kept values doubled, dropped ones zero), identically on any device.

    Seed, step and rank enter the kernels from device memory and launch arguments only, so the stream works inside
    ``TrainStep(graph=True)`` / ``FlatTrainStep(graph=True)`` and every replay advances the step.  ``rank`` separates the
    masks of data-parallel replicas (0 .. 2^28 - 1).  ``detach()`` restores the heads' plain ``F.dropout`` path."""

    HEADS = ("pose_calculator_4", "pose_warp_refinement_3.pose_calculator", "pose_warp_refinement_2.pose_calculator",
             "pose_warp_refinement_1.pose_calculator")        # forward order: head 0 .. 3 of the counter

    def __init__(self, net, seed=0, rank=0):
        seed, rank = int(seed), int(rank)
        if not -(1 << 63) <= seed < (1 << 64):
            raise ValueError("dropout stream: seed=%d does not fit 64 bits" % seed)
        if not 0 <= rank < (1 << 28):
            raise ValueError("dropout stream: rank=%d outside [0, 2^28)" % rank)
        self.seed, self.rank = seed & ((1 << 64) - 1), rank
        self._step_host = 0
        self._state = None
        self._log = None
        self.net = None
        self.attach(net)

    # ---- attachment ----------------------------------------------------------------------------------------------------
    def attach(self, net):
        if self.net is not None:
            raise RuntimeError("dropout stream: already attached (detach() first)")
        if not hasattr(net, "get_submodule"):
            raise TypeError("dropout stream: needs the PWCLONet module, got %s" % type(net).__name__)
        try:
            heads = [net.get_submodule(name) for name in self.HEADS]
        except AttributeError as e:
            raise TypeError("dropout stream: the module has no pose head %s" % e) from e
        if any(not hasattr(h, "from_logits") for h in heads):
            raise TypeError("dropout stream: the pose heads must be this package's PoseCalculator")
        if getattr(net, "_dropout_stream", None) is not None:
            raise RuntimeError("dropout stream: the network already has a stream attached")
        for i, h in enumerate(heads):
            h._dropout_stream = (self, i)
        net._dropout_stream = self
        self.net = net
        first = next(net.parameters(), None)
        if first is not None and first.is_cuda:
            self.state_on(first.device)          # made here, outside any capture
        return self

    def detach(self):
        """Today's behaviour again: the heads call ``F.dropout`` and no begin launch is issued."""
        if self.net is not None:
            for name in self.HEADS:
                self.net.get_submodule(name)._dropout_stream = None
            self.net._dropout_stream = None
            self.net = None

    # ---- device state (used by the network and the heads) ---------------------------------------------------------------
    def state_on(self, device):
        """The (3,) int64 device state {seed, next step, step in flight}, made on first use."""
        if self._state is None or self._state.device != device:
            if self._state is not None:
                self._step_host = int(self._state[1].item())
            signed = self.seed - (1 << 64) if self.seed >= (1 << 63) else self.seed
            self._state = torch.tensor([signed, self._step_host, self._step_host], dtype=torch.int64).to(device)
            self._log = None
        return self._state

    def keep_log(self, head, batch, device):
        """Head ``head``'s (B,256) uint8 slot of the record ``masks()`` reads."""
        if self._log is None or self._log.shape[1] != batch or self._log.device != device:
            self._log = torch.zeros((4, batch, 256), dtype=torch.uint8, device=device)
        return self._log[head]

    def begin(self, device):
        """One launch: step in flight = next step, next step += 1."""
        _lib.call("pose_head_train_begin_kernel_wrapper", device, self.state_on(device).data_ptr())

    # ---- the step counter ------------------------------------------------------------------------------------------------
    def step_index(self):
        """The step the next training forward (or replay) will use."""
        return self._step_host if self._state is None else int(self._state[1].item())

    def set_step(self, k):
        k = int(k)
        if not 0 <= k < (1 << 62):
            raise ValueError("dropout stream: step=%d outside [0, 2^62)" % k)
        self._step_host = k
        if self._state is not None:
            self._state[1:2].fill_(k)

    def masks(self):
        """(4, 2, B, 256) bool: the keep masks of the last training forward -- [head, branch (0 = q, 1 = t), cloud, unit]."""
        if self._log is None:
            raise RuntimeError("dropout stream: no training forward has run yet")
        return torch.stack(((self._log & 1) != 0, (self._log & 2) != 0), dim=1)

    def state_dict(self):
        return {"seed": self.seed, "rank": self.rank, "step": self.step_index()}

    def load_state_dict(self, sd):
        """Seed and step are written to the device state, which a captured graph re-reads; the rank is a launch argument:
        load it before capturing."""
        seed, rank = int(sd["seed"]), int(sd["rank"])
        if not -(1 << 63) <= seed < (1 << 64):
            raise ValueError("dropout stream: seed=%d does not fit 64 bits" % seed)
        if not 0 <= rank < (1 << 28):
            raise ValueError("dropout stream: rank=%d outside [0, 2^28)" % rank)
        self.seed, self.rank = seed & ((1 << 64) - 1), rank
        self.set_step(sd["step"])
        if self._state is not None:
            self._state[0:1].fill_(self.seed - (1 << 64) if self.seed >= (1 << 63) else self.seed)
