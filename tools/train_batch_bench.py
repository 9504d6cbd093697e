#!/usr/bin/env python3
"""Time of one training batch built from raw LiDAR pairs on the device (batches.TrainBatchBuilder).

    python tools/train_batch_bench.py [--batch 32] [--repeats 7] [--inner 5] [--out profiles/train_batch/bench.json]

One process, every variant timed ``--repeats`` times in alternation (variant A, B, C, ..., then again), ``--inner``
batches per timing between two device synchronisations; median and min / max of the repeats are reported:

* builder, augmentation on: eager and as one hipGraph;
* builder with ``augment=False``: eager and as one hipGraph;
* the only way to make the same batch without the builder: 2B calls of ``preprocess.kitti_frame_to_cloud(sample="random")``
  on the same 2B KITTI frames (no augmentation, no ground truth: compare with ``augment=False``);
* the graphed ``TrainStep`` alone, and with the builder graph replayed in front of it into the step's static tensors
  (skipped with ``--no-train-step``).

Synthetic raw-sized sweeps (``batches.synthetic_raw_pairs``: 64-beam ray casts of 2048 azimuth steps, padded to the
capacity); KITTI conventions.  Prints one JSON line."""
import argparse, json, os, statistics, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pwclonet_pylidarslam_amd import batches, preprocess  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--npoints", type=int, default=8192)
    ap.add_argument("--capacity", type=int, default=131072)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--no-train-step", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    assert a.repeats >= 7, "at least 7 repeats: the spread is part of the result"
    dev = torch.device("cuda", 0)
    B, m = a.batch, a.npoints
    sweeps, lengths, t_diff = batches.synthetic_raw_pairs(B, seed=17, capacity=a.capacity)
    sweeps, dlen, t_diff = sweeps.to(dev), lengths.to(dev), t_diff.to(dev)
    tr = batches.VELO_TO_CAM
    variants = {}

    def builder_variants(tag, augment, out=None):
        bld = batches.TrainBatchBuilder(B, dataset="kitti", npoints=m, capacity=a.capacity, augment=augment, seed=1, tr=tr)
        bld.build(sweeps, dlen, t_diff, out=out)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            bld.build(sweeps, dlen, t_diff, out=out)
        variants["builder_%s_eager" % tag] = lambda: bld.build(sweeps, dlen, t_diff, out=out)
        variants["builder_%s_graph" % tag] = g.replay
        return bld, g

    bld, _ = builder_variants("augment", True)
    builder_variants("noaug", False)
    counts = bld.survivor_counts().cpu()
    n_rows = lengths.min(dim=1).values

    def per_frame():                                       # what the package offered before the builder
        for b in range(B):
            n = int(n_rows[b])
            for f in range(2):
                preprocess.kitti_frame_to_cloud(sweeps[b, f, :n], tr, m, sample="random")
    variants["per_frame_kitti_frame_to_cloud"] = per_frame

    if not a.no_train_step:
        from pwclonet_pylidarslam_amd.loss import PWCLONetLossModule
        from pwclonet_pylidarslam_amd.pwclonet import PWCLONet
        from pwclonet_pylidarslam_amd.training import PWCLONetWithLoss, TrainStep
        torch.manual_seed(7)
        net = PWCLONet(dict(num_input_channels=3, sequence_len=2, device=str(dev), scalar_last=False,
                            log_mode="none")).to(dev).train()
        loss_mod = PWCLONetLossModule(dict(with_exp_weights=True, init_weights=[0.0, -2.5], loss_option="l2_norm",
                                           nb_levels=4, scalar_last=False)).to(dev)
        unit = PWCLONetWithLoss(net, loss_mod)
        opt = torch.optim.Adam(unit.parameters(), lr=1e-4, capturable=True, fused=True)
        static = tuple(t.clone() for t in bld.build(sweeps, dlen, t_diff))
        ts = TrainStep(unit, opt, *static, graph=True)
        feed = batches.TrainBatchBuilder(B, dataset="kitti", npoints=m, capacity=a.capacity, seed=2, tr=tr)
        feed.build(sweeps, dlen, t_diff, out=static)
        torch.cuda.synchronize()
        fg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(fg):
            feed.build(sweeps, dlen, t_diff, out=static)
        variants["train_step_graph"] = ts.step

        def fed_step():
            fg.replay()
            ts.step()
        variants["builder_graph_then_train_step_graph"] = fed_step

    for fn in variants.values():                           # warm-up of every variant
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.repeats):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.inner):
                fn()
            torch.cuda.synchronize()
            times[k].append(1e3 * (time.perf_counter() - t0) / a.inner)
    res = {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
           for k, v in times.items()}
    line = {"metric": "training batch from raw LiDAR pairs, ms per batch of %d pairs (2 x %d points from ~%d raw rows each)"
                      % (B, m, int(n_rows.float().mean())),
            "value": res["builder_augment_graph"]["median_ms"], "unit": "ms/batch", "batch": B, "npoints": m,
            "capacity": a.capacity, "rows_min_max": [int(n_rows.min()), int(n_rows.max())],
            "survivors_min_max": [int(counts.min()), int(counts.max())], "repeats": a.repeats, "inner": a.inner,
            "device": torch.cuda.get_device_name(0), "variants": res}
    if "train_step_graph" in res:
        line["builder_in_front_of_step_ms"] = round(res["builder_graph_then_train_step_graph"]["median_ms"]
                                                    - res["train_step_graph"]["median_ms"], 4)
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
