"""The data-parallel training step as replayable graphs: one flat gradient bucket, one HIP Adam.

``DistributedDataParallel``'s bucket hooks and ``torch.optim.Adam`` walk the unit's 330 tensors through host-driven
code, which a captured graph cannot hold.  Here the 775 070 gradients (3.1 MB) are gathered into ONE buffer by
``csrc/flat_step.hip``'s pack kernel, that buffer is all-reduced by a plain eager collective, and one Adam launch
group steps every parameter from it:

    graph 1: zero_grad -> forward -> loss -> backward -> pack(1 / world)
    eager  : dist.all_reduce(bucket, SUM)
    graph 2: Adam

The collective is never captured.  There is no fall-back: CPU tensors are refused, a missing kernel is an error.
"""
import ctypes

import torch

from . import _lib

ALIGN_VALUES = 64          # csrc/flat_step.hip FLAT_ALIGN: every bucket offset is a multiple (256 bytes)


def bucket_layout(sizes, align_values=ALIGN_VALUES):
    """``(offsets, total)`` of tensors of ``sizes`` values laid back to back, each at a multiple of ``align_values``
    values; ``total`` = the last tensor's end rounded up, plus ONE value at the very end: the non-finite count."""
    if align_values < 1:
        raise ValueError("align_values must be positive, got %r" % (align_values,))
    offsets, end = [], 0
    for s in sizes:
        if s < 0:
            raise ValueError("negative tensor size %r" % (s,))
        offsets.append(end)
        end += -(-int(s) // align_values) * align_values
    return offsets, end + 1


def refuse_other_optimizers(optimizer_type):
    """The reference's trainer offers adam / adamw / sgd / rmsprop; only the first two have a flat kernel.  Returns the
    ``decoupled`` flag of ``FlatAdam`` for them."""
    kind = str(optimizer_type).lower()
    if kind in ("adam", "adamw"):
        return kind == "adamw"
    raise NotImplementedError("FlatAdam implements optimizer_type 'adam' and 'adamw' only; %r (SGD, RMSprop, ...) has no "
                              "flat kernel: train it with torch.optim and training.TrainStep" % (optimizer_type,))


class FlatAdam:
    """``torch.optim.Adam`` (``decoupled=False``: ``weight_decay`` is L2, added to the gradient) or ``AdamW``
    (``decoupled=True``) over ``params``, without amsgrad / maximize, as one launch group of ``csrc/flat_step.hip``.

    Owns the flat gradient ``bucket`` (``total`` fp32 values, the last one the count of non-finite gradient values of
    the last ``pack`` -- ``nonfinite`` is a view of it), the two moment buffers at the same offsets, and the device
    scalars ``step_count`` (int64), ``skipped`` (int64) and ``lr`` (float64).  The parameters are neither re-pointed nor
    copied: the model and its ``state_dict`` stay as they are.  ``step()`` applies nothing -- parameters, moments and
    counter keep their bits -- while the count is not zero (the reference raises on a NaN loss; a replayed graph cannot)
    and adds 1 to ``skipped``, which no ``pack()`` resets: read it once after an epoch of replays."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False):
        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("FlatAdam got no parameter that requires a gradient")
        for p in self.params:
            if not p.is_cuda:
                raise RuntimeError("CPU not supported")
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("FlatAdam parameters must be contiguous float32 tensors")
            if p.device != self.params[0].device:
                raise RuntimeError("FlatAdam parameters must live on one device")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0 and eps >= 0.0 and weight_decay >= 0.0 and lr >= 0.0):
            raise ValueError("invalid Adam hyper-parameters: lr=%r betas=%r eps=%r weight_decay=%r"
                             % (lr, betas, eps, weight_decay))
        self.device = dev = self.params[0].device
        self.betas, self.eps, self.weight_decay = (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.decoupled = bool(decoupled)
        self.sizes = [p.numel() for p in self.params]
        self.offsets, self.total = bucket_layout(self.sizes)
        self.bucket = torch.zeros(self.total, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros_like(self.bucket)
        self.exp_avg_sq = torch.zeros_like(self.bucket)
        self.nonfinite = self.bucket[self.total - 1:]
        self.step_count = torch.zeros(1, dtype=torch.int64, device=dev)
        self.skipped = torch.zeros(1, dtype=torch.int64, device=dev)
        self.lr = torch.full((1,), float(lr), dtype=torch.float64, device=dev)
        self._lr_host = float(lr)
        self._coef = torch.zeros(4, dtype=torch.float64, device=dev)
        n = len(self.params)
        ll = ctypes.c_longlong * n
        self._counts, self._offsets = ll(*self.sizes), ll(*self.offsets)
        self._param_ptrs = (ctypes.c_void_p * n)(*[p.data_ptr() for p in self.params])

    # ---- the two launch groups -------------------------------------------------------------------------------------

    def pack(self, scale=1.0):
        """Gather the current ``p.grad`` tensors into the bucket, times ``scale`` (1 / world; exactly 1.0 keeps the
        bits), and count their non-finite values into the last slot."""
        grads = []
        for p in self.params:
            g = p.grad
            if g is None:
                raise RuntimeError("FlatAdam.pack: a parameter has no gradient (every parameter of the unit takes part "
                                   "in the step)")
            if not g.is_cuda:
                raise RuntimeError("CPU not supported")
            if g.dtype != torch.float32 or not g.is_contiguous() or g.numel() != p.numel():
                raise RuntimeError("FlatAdam.pack: gradients must be contiguous float32 tensors of the parameter's size")
            grads.append(g.data_ptr())
        n = len(grads)
        _lib.call("flat_pack_kernel_wrapper", self.device, n, (ctypes.c_void_p * n)(*grads), self._counts, self._offsets,
                  float(scale), self.bucket.data_ptr(), self.total)

    def step(self):
        """One Adam update of every parameter from the bucket (skipped as a whole while ``nonfinite`` is not zero)."""
        _lib.call("flat_adam_skipped_kernel_wrapper", self.device, len(self.params), self._param_ptrs, self._counts,
                  self._offsets, self.bucket.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.total,
                  self.step_count.data_ptr(), self.lr.data_ptr(), self._coef.data_ptr(), self.betas[0], self.betas[1],
                  self.eps, self.weight_decay, int(self.decoupled), self.skipped.data_ptr())

    def set_lr(self, lr):
        """Write the device scalar the kernel reads: a schedule needs no recapture."""
        self._lr_host = float(lr)
        self.lr.fill_(self._lr_host)

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def view(self, flat, i):
        """Tensor ``i``'s part of a flat buffer (bucket, exp_avg, exp_avg_sq), shaped like the parameter."""
        return flat[self.offsets[i]:self.offsets[i] + self.sizes[i]].view_as(self.params[i])

    # ---- torch.optim.Adam's checkpoint layout ------------------------------------------------------------------------

    def state_dict(self):
        """``torch.optim.Adam.state_dict()``'s layout: per-parameter ``step`` / ``exp_avg`` / ``exp_avg_sq`` and one
        parameter group; ``torch.optim.Adam(...).load_state_dict`` accepts it (and carries the group's extra
        ``flat_skipped`` entry, the cumulative skipped-step count, along without reading it)."""
        step = int(self.step_count.item())
        state = {}
        if step > 0:
            for i in range(len(self.params)):
                state[i] = {"step": torch.tensor(float(step), dtype=torch.float32),
                            "exp_avg": self.view(self.exp_avg, i).clone(),
                            "exp_avg_sq": self.view(self.exp_avg_sq, i).clone()}
        group = {"lr": self._lr_host, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay,
                 "amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False,
                 "fused": None, "decoupled_weight_decay": self.decoupled, "flat_skipped": int(self.skipped.item()),
                 "params": list(range(len(self.params)))}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        """Resume from ``torch.optim.Adam`` / ``AdamW`` / ``FlatAdam.state_dict()``.  Several parameter groups (the
        reference's trainer builds two) are accepted when they share their hyper-parameters."""
        groups = sd["param_groups"]
        order = [i for g in groups for i in g["params"]]
        if len(order) != len(self.params):
            raise ValueError("the checkpoint holds %d parameters, this optimizer %d" % (len(order), len(self.params)))
        g0 = groups[0]
        key = lambda g: (float(g["lr"]), tuple(float(b) for b in g["betas"]), float(g["eps"]), float(g["weight_decay"]),
                         bool(g.get("decoupled_weight_decay", False)))
        if any(key(g) != key(g0) for g in groups[1:]):
            raise ValueError("FlatAdam steps every parameter with ONE set of hyper-parameters; the checkpoint's groups differ")
        if any(g.get("amsgrad", False) or g.get("maximize", False) for g in groups):
            raise NotImplementedError("FlatAdam has no amsgrad / maximize variant")
        self.betas, self.eps = (float(g0["betas"][0]), float(g0["betas"][1])), float(g0["eps"])
        self.weight_decay = float(g0["weight_decay"])
        if "decoupled_weight_decay" in g0:
            self.decoupled = bool(g0["decoupled_weight_decay"])
        self.set_lr(g0["lr"])
        state, steps = sd["state"], set()
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        for i, k in enumerate(order):
            st = state.get(k)
            if st is None:
                steps.add(0)
                continue
            steps.add(int(float(st["step"])))
            for flat, name in ((self.exp_avg, "exp_avg"), (self.exp_avg_sq, "exp_avg_sq")):
                src = st[name]
                if src.numel() != self.sizes[i]:
                    raise ValueError("checkpoint tensor %d has %d values, the parameter %d" % (k, src.numel(), self.sizes[i]))
                self.view(flat, i).copy_(src.reshape(self.params[i].shape))
        if len(steps) > 1:
            raise ValueError("FlatAdam keeps ONE step counter; the checkpoint's parameters are at steps %s" % sorted(steps))
        self.step_count.fill_(steps.pop() if steps else 0)
        self.skipped.fill_(int(g0.get("flat_skipped", 0)))         # (torch's own checkpoints have no such entry)


class FlatTrainStep:
    """One data-parallel training step of the bare ``PWCLONetWithLoss`` unit (NOT DDP-wrapped) with ``FlatAdam``:

        gradients set to none -> forward -> loss -> backward -> ``pack(1 / world)``
        -> ``dist.all_reduce(bucket, SUM)`` when ``process_group`` is given (also at world size 1)
        -> the Adam launch group.

    ``graph=True``: everything before the all-reduce is one captured graph and the Adam launch group a second one; the
    all-reduce runs eagerly between the two replays on the current stream and is never captured.  With
    ``process_group=None`` there is no collective and the whole step is a single graph.  With a process group the
    parameters are broadcast from its rank 0 once, here.  ``step()`` returns the loss tensor (static under the graph:
    read it before the next replay).

    The ``warmup`` steps before the capture (allocator, autograd and communicator warm-up, on a side stream as
    ``TrainStep`` does it) are REAL updates: parameters, moments, BatchNorm statistics and the step counter move, so after
    ``k`` calls of ``step()`` the counter reads ``warmup + k``.  Reload the state afterwards to start from it."""

    def __init__(self, model, optimizer, xyz_f1, xyz_f2, gt_params, graph=False, process_group=None, warmup=3):
        if not isinstance(optimizer, FlatAdam):
            raise TypeError("FlatTrainStep needs a FlatAdam (torch optimizers go with training.TrainStep)")
        if hasattr(model, "module"):
            raise TypeError("FlatTrainStep takes the bare unit: its bucket replaces DistributedDataParallel")
        self.model, self.opt, self.group = model, optimizer, process_group
        self.args = (xyz_f1, xyz_f2, gt_params)
        self.front = self.back = None
        self.world = 1
        if process_group is not None:
            import torch.distributed as dist
            self.world = dist.get_world_size(process_group)
            src = dist.get_global_rank(process_group, 0)
            for p in optimizer.params:
                dist.broadcast(p.data, src=src, group=process_group)
        self.scale = 1.0 / self.world
        if graph:
            dev = xyz_f1.device
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(warmup):
                    self._eager()
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
            self.opt.zero_grad(set_to_none=True)
            self.front = torch.cuda.CUDAGraph()
            with _lib.capture(self.front, **self.capture_kw(process_group)):
                self.static_loss = self._front()
                if process_group is None:
                    self.opt.step()
            if process_group is not None:
                self.back = torch.cuda.CUDAGraph()
                with _lib.capture(self.back, **self.capture_kw(process_group)):
                    self.opt.step()
            torch.cuda.synchronize(dev)

    @staticmethod
    def capture_kw(process_group):
        """Keyword arguments of ``torch.cuda.graph`` for a capture made while a process group is alive.  The RCCL process
        group's watchdog THREAD polls the events of the collectives already issued (the construction broadcast, the
        warm-up all-reduces) with ``hipEventQuery``; under the default capture mode ("global") HIP refuses that call on
        any thread while a capture is open, the watchdog throws and the process aborts.  "thread_local" restricts the
        check to the capturing thread, which issues no collective inside the capture."""
        return {} if process_group is None else {"capture_error_mode": "thread_local"}

    def _front(self):
        self.opt.zero_grad(set_to_none=True)
        loss, _pose, _log = self.model(*self.args)
        loss.backward()
        self.opt.pack(self.scale)
        return loss

    def _reduce(self):
        import torch.distributed as dist
        dist.all_reduce(self.opt.bucket, op=dist.ReduceOp.SUM, group=self.group)

    def _eager(self):
        loss = self._front()
        if self.group is not None:
            self._reduce()
        self.opt.step()
        return loss

    def step(self):
        if self.front is None:
            return self._eager()
        self.front.replay()
        if self.back is not None:
            self._reduce()
            self.back.replay()
        return self.static_loss
