#!/usr/bin/env python3
"""Training-step throughput of PWCLO-Net on the HIP ops (BASELINE.json configs[3]).

    python tools/train_step.py [--batch 8] [--steps 10]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 tools/train_step.py --gpus N
    python tools/train_step.py --flat --graph [--gpus N]
    python tools/train_step.py --graph --fused-adam --dropout-stream [SEED]
    python tools/train_step.py --flat --graph --bn-cell --epochs 3 --steps-per-epoch 10

One process per GPU; the reference-shaped module graph in TRAIN mode (BatchNorm batch statistics,
dropout; torch conv/BN autograd + the HIP gather/group forward and backward kernels), the
reference's supervised loss (pwclonet_pylidarslam_amd.loss), Adam, and -- for N > 1 --
DistributedDataParallel over RCCL: one 3.1 MB gradient all-reduce per step, BN buffers not
broadcast.  --flat replaces DDP + torch's Adam by flat_step.FlatAdam / FlatTrainStep: one flat gradient bucket, one
eager all-reduce, one HIP Adam launch group -- the data-parallel step that replays as graphs (--gpus N --graph).
Not the headline benchmark (bench.py measures forward pairs/s); prints one JSON line.
"""
import argparse, json, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pwclonet_pylidarslam_amd  # noqa: E402,F401
pwclonet_pylidarslam_amd.configure_hw_queues(8)
import torch  # noqa: E402

import bench  # noqa: E402
from pwclonet_pylidarslam_amd import dist_util  # noqa: E402
from pwclonet_pylidarslam_amd.loss import PWCLONetLossModule  # noqa: E402
from pwclonet_pylidarslam_amd.pointnet2_ops.pytorch_utils import BNMomentumScheduler, attach_bn_momentum  # noqa: E402
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet  # noqa: E402
from pwclonet_pylidarslam_amd.training import (DropoutStream, EpochSchedule, FlatAdam, FlatTrainStep, PWCLONetWithLoss,  # noqa: E402
                                               TrainStep, ddp_wrap, gradient_bucket_values)


def _momentum(model):
    """The BatchNorm layers' common momentum."""
    values = {m.momentum for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)}
    assert len(values) == 1, values
    return values.pop()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--batch", type=int, default=8, help="frame pairs per GPU per step")
    ap.add_argument("--npoints", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--fused-adam", action="store_true", help="torch.optim.Adam(fused=True): one multi-tensor kernel")
    ap.add_argument("--graph", action="store_true",
                    help="capture forward + loss + backward + Adam into one hipGraph (single GPU only)")
    ap.add_argument("--flat", action="store_true",
                    help="flat_step.FlatAdam + FlatTrainStep: flat gradient bucket, eager all-reduce, HIP Adam; with it --graph "
                         "is allowed for --gpus N (two graphs around the collective); --gpus 1 runs the world-1 collective too")
    ap.add_argument("--sample-ahead", action="store_true",
                    help="draw the next batch's furthest-point samples on a second stream while this batch's step runs "
                         "(training.TrainStep(sample_ahead=True); the synthetic batch is the same every step)")
    ap.add_argument("--raw-batches", action="store_true",
                    help="every step trains on a fresh batch built from raw synthetic sweeps by batches.TrainBatchBuilder "
                         "(filter, random choice, augmentation, ground truth on the device), written into the step's tensors")
    ap.add_argument("--dropout-stream", type=int, nargs="?", const=0, default=None, metavar="SEED",
                    help="training.DropoutStream(net, seed=SEED, rank=rank): replayable dropout masks and the pose heads as "
                         "hand-written kernels (without it the heads call F.dropout: torch's stream)")
    ap.add_argument("--bn-cell", action="store_true",
                    help="pytorch_utils.attach_bn_momentum before the step is built: the training kernels read the BatchNorm "
                         "momentum from device memory, so replays follow the momentum schedule")
    ap.add_argument("--epochs", type=int, default=0,
                    help="with --steps-per-epoch K: time E blocks of K steps with training.EpochSchedule.epoch_end() between "
                         "them (the reference's BatchNorm momentum lambda stepping every epoch, MultiStepLR(milestones=[1, 2], gamma=0.5)) "
                         "instead of --steps steps")
    ap.add_argument("--steps-per-epoch", type=int, default=10)
    a = ap.parse_args()
    if a.gpus > 1 and not dist_util.launched_by_torchrun():      # supervise N fresh ranks; no GPU call made here
        sys.exit(dist_util.spawn_ranks(os.path.abspath(__file__), sys.argv[1:], a.gpus))
    explicit_gpus = any(x == "--gpus" or x.startswith("--gpus=") for x in sys.argv[1:])
    rank, local_rank, world = dist_util.env_world()
    assert world == a.gpus, "WORLD_SIZE=%d but --gpus %d" % (world, a.gpus)
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    dist_util.init("nccl", dev)
    torch.manual_seed(7)                                   # same initial weights on every rank
    net = PWCLONet(dict(num_input_channels=3, sequence_len=2, device=str(dev), scalar_last=False,
                        log_mode="none")).to(dev).train()
    loss_mod = PWCLONetLossModule(dict(with_exp_weights=True, init_weights=[0.0, -2.5], loss_option="l2_norm",
                                       nb_levels=4, scalar_last=False)).to(dev)
    # network + loss in ONE module: the all-reduce carries the 775 068 network gradients and the loss module's two
    # learnable weights -- with the network alone under DDP the replicas' loss weights drift
    unit = PWCLONetWithLoss(net, loss_mod)
    stream = DropoutStream(net, seed=a.dropout_stream, rank=rank) if a.dropout_stream is not None else None
    cell = attach_bn_momentum(unit) if a.bn_cell else None
    group = None
    if a.flat:
        assert not (a.fused_adam or a.sample_ahead), "--flat brings its own Adam kernel; not combined with --fused-adam / --sample-ahead"
        if explicit_gpus:                                  # --gpus given: the collective runs, also at world size 1
            import torch.distributed as dist
            if not dist.is_initialized():
                os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
                os.environ.setdefault("MASTER_PORT", "29533")
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
            group = dist.group.WORLD
        model, opt = unit, FlatAdam(unit.parameters(), lr=1e-4)
    else:
        model = ddp_wrap(unit, dev) if world > 1 else unit
        opt = torch.optim.Adam(unit.parameters(), lr=1e-4, capturable=a.graph, fused=True if a.fused_adam else None)
    schedule = None
    if a.epochs:
        assert not a.graph or (a.flat and a.bn_cell), \
            "--epochs with --graph needs --flat (a device learning rate) and --bn-cell (a device momentum): replays ignore the rest"
        from torch.optim.lr_scheduler import MultiStepLR
        # the reference's lambda (train.py:322; init 0.5, rate 0.5, max 0.99) with a decay step of ONE epoch: a short run moves
        bn_sched = BNMomentumScheduler(unit, lambda it: min(1 - 0.5 * 0.5 ** int(it / 1), 0.99))
        schedule = EpochSchedule(opt, lambda o: MultiStepLR(o, milestones=[1, 2], gamma=0.5), bn_sched)
        a.steps = a.epochs * a.steps_per_epoch
    x1, x2 = bench.make_batch(a.batch, a.npoints, 2000 + rank, dev)
    g = torch.Generator().manual_seed(3 + rank)
    gt = torch.randn(a.batch, 7, generator=g) * 0.1
    gt[:, 3:] = torch.nn.functional.normalize(gt[:, 3:] + torch.tensor([1.0, 0, 0, 0]), dim=1)
    gt = gt.to(dev)

    if a.flat:
        step = FlatTrainStep(unit, opt, x1, x2, gt, graph=a.graph, process_group=group).step
    else:
        if a.graph:
            assert world == 1, "--graph is the single-GPU variant (DDP's bucketed all-reduce is not captured here; --flat is)"
        step = TrainStep(model, opt, x1, x2, gt, graph=a.graph, sample_ahead=a.sample_ahead).step
    if a.raw_batches:
        assert not a.sample_ahead, "--raw-batches rewrites the step's tensors every step; not combined with --sample-ahead"
        from pwclonet_pylidarslam_amd import batches
        assert a.npoints <= batches.MAX_NPOINTS
        sweeps, lengths, t_diff = (t.to(dev) for t in batches.synthetic_raw_pairs(a.batch, seed=2000 + rank))
        builder = batches.TrainBatchBuilder(a.batch, dataset="kitti", npoints=a.npoints, seed=rank, tr=batches.VELO_TO_CAM)
        feed = lambda: builder.build(sweeps, lengths, t_diff, out=(x1, x2, gt))
        feed()
        if a.graph:                                        # one capture serves every step: the counter lives on the device
            torch.cuda.synchronize(dev)
            feed_graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(feed_graph, **(FlatTrainStep.capture_kw(group) if a.flat else {})):
                feed()
            feed = feed_graph.replay
        train = step

        def step():
            feed()
            return train()

    losses = [step().item() for _ in range(a.warmup)]
    dist_util.fence(dev)
    t0 = time.perf_counter()
    for k in range(a.steps):
        if schedule is not None and k and k % a.steps_per_epoch == 0:
            schedule.epoch_end()
        loss = step()
    dist_util.fence(dev)
    dt = dist_util.max_over_ranks(time.perf_counter() - t0, dev)
    losses.append(loss.item())
    if rank == 0:
        print(json.dumps({"metric": "PWCLO-Net training frame-pairs/sec (fwd+bwd+Adam), 2x%d-pt pairs" % a.npoints,
                          "value": world * a.batch * a.steps / dt, "unit": "frame-pairs/s", "n_gpus": world,
                          "ms_per_step": 1e3 * dt / a.steps, "batch_per_gpu": a.batch, "dtype": "f32",
                          "launch": (("two hipGraphs per step around the eager all-reduce" if a.flat and group is not None
                                      else "one hipGraph per step") if a.graph else "eager (module graph, torch autograd)")
                          + (", flat gradient bucket + HIP Adam" if a.flat else "")
                          + (", next batch's sampling chain on a second stream" if a.sample_ahead else "")
                          + (", every batch built from raw sweeps on the device" if a.raw_batches else ""),
                          "dropout": ("DropoutStream(seed=%d): counter-based masks, HIP pose heads, next step %d"
                                      % (a.dropout_stream, stream.step_index())) if stream is not None else "F.dropout",
                          "loss_first_last": [losses[0], losses[-1]],
                          "skipped": int(opt.skipped.item()) if a.flat else None,
                          "bn_momentum": _momentum(unit), "bn_cell": cell is not None,
                          "epoch_ends": schedule.epoch if schedule is not None else 0,
                          "collective": ("eager all-reduce of the flat bucket (%d fp32 values: %d gradients, padding, the "
                                         "non-finite count), world size %d" % (opt.total, gradient_bucket_values(unit), world))
                          if group is not None else
                          ("DDP all-reduce of %d fp32 gradient values (network + loss weights), one bucket"
                           % gradient_bucket_values(unit)) if world > 1 else "none"}), flush=True)
    dist_util.finish()


if __name__ == "__main__":
    main()
