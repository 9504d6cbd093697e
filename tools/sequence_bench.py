#!/usr/bin/env python3
"""Sequence odometry against pair mode, both shapes, one process, alternated and repeated; prints one JSON line.

configs[2] shape: fp32, 8192 points.  Pair mode = bench.py's headline loop (batch 32, ``PipelinedForward`` with 4 in
flight); sequence mode = ``PipelinedSequence`` (33-frame windows, 4 slots) over one long device sequence, so a timed
region of K steps is K windows = 32 K pairs on both sides.  The long sequence alternates one synthetic 33-frame
sequence forwards and backwards (window 2k = the sequence, window 2k+1 = it reversed: every window is a real
consecutive-frame window of the same cloud sizes).  Check: the rows of window 0 equal pair mode's poses of the same 32
pairs bit for bit.

configs[4] shape: bf16, raw ~120k-row KITTI-360-like frames -> filter -> compaction -> exact sampling to 8192 ->
pyramid, eager (as ``bench.py --config 5``).  Pair step = ``run_config5``'s 16 raw frames (8 pairs); sequence step = 9
raw frames -> the same 8 pairs.  1 and 2 steps in flight; with 2, the large-cloud sampler's plain launch and the
spatial-order choice of ``run_config5`` on both sides (at most two sampler launches of <= 128 workgroups in flight).
Check: both sides' poses of the same pairs are equal bit for bit.

    python tools/sequence_bench.py [--steps K] [--warmup W] [--repeats R] [--shapes 2,4] [--dry]

``--dry``: builds the inputs and the net on the host and stops before the first device call.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import pwclonet_pylidarslam_amd  # noqa: E402
from pwclonet_pylidarslam_amd import _lib, synthetic  # noqa: E402
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet  # noqa: E402


def _net(dev, dtype):
    torch.manual_seed(1234)
    net = PWCLONet(dict(num_input_channels=3, sequence_len=2, device=str(dev), scalar_last=False,
                        log_mode="none")).to(dev).eval()
    return net.prepare_fused(dtype=dtype)


def _stats(pairs, times):
    rates = sorted(pairs / t for t in times)
    med = rates[len(rates) // 2]
    return {"median": med, "min": rates[0], "max": rates[-1], "spread_pct": 100.0 * (rates[-1] - rates[0]) / med,
            "all": rates}


def _timed(dev, fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def shape2(args, dev, base):
    """base: (33, N, 4) host frames of one synthetic sequence."""
    from pwclonet_pylidarslam_amd.graphed import PipelinedForward, PipelinedSequence
    T = base.shape[0]
    P = T - 1
    K = args.steps
    fwd = torch.from_numpy(base)
    # window 2k = base, window 2k+1 = base reversed; windows share their boundary frame
    parts = [fwd] + [(fwd.flip(0) if k % 2 == 0 else fwd)[1:] for k in range(K - 1)]
    long_seq = torch.cat(parts).contiguous()
    assert long_seq.shape[0] == K * P + 1
    cm = lambda z: z[:, :, :3].permute(0, 2, 1).contiguous()
    x1, x2 = cm(fwd[:-1]), cm(fwd[1:])
    if args.dry:
        return {"dry": True, "frames": int(long_seq.shape[0])}
    net = _net(dev, "f32")
    long_seq, x1, x2 = long_seq.to(dev), x1.to(dev), x2.to(dev)
    pipe = PipelinedForward(net, depth=args.inflight)
    pipe.prepare(x1, x2)
    seq = PipelinedSequence(net, window=T, depth=args.inflight, streams=pipe.streams)   # one set of streams per process
    seq(long_seq[:args.inflight * P + 1])                       # captures every slot (set-up, not timed)
    torch.cuda.synchronize(dev)

    def run_pairs(k):
        out = None
        for _ in range(k):
            out = pipe(x1, x2)[0]
        return out

    def run_seq(frames):
        return seq(frames)

    for _ in range(args.warmup):
        run_pairs(1)
        run_seq(long_seq[:P + 1])
    t_pair, t_seq = [], []
    for _ in range(args.repeats):                               # alternated
        dt, pose_pair = _timed(dev, lambda: run_pairs(K))
        t_pair.append(dt)
        dt, rows = _timed(dev, lambda: run_seq(long_seq))
        t_seq.append(dt)
    _lib.synchronize(dev)
    eager_last, _ = net.forward_sequence(long_seq[-T:]) if K > 1 else (None, None)
    bitwise = bool(torch.equal(rows[:P], pose_pair))
    last_ok = eager_last is None or bool(torch.equal(rows[-P:], eager_last))
    ps, ss = _stats(K * P, t_pair), _stats(K * P, t_seq)
    return {"workload": "BASELINE.json configs[2] shape: synthetic KITTI-like sequence, %d points, fp32" % base.shape[1],
            "pair": {"mode": "PipelinedForward, batch %d, %d in flight (bench.py's loop)" % (P, args.inflight),
                     "frame_pairs_per_s": ps, "ms_per_%d_pairs" % P: 1e3 * sorted(t_pair)[len(t_pair) // 2] / K},
            "sequence": {"mode": "PipelinedSequence, %d-frame windows overlapping by one frame, %d slots, one %d-frame "
                                 "sequence per timed region" % (T, args.inflight, long_seq.shape[0]),
                         "frame_pairs_per_s": ss, "ms_per_%d_pairs" % P: 1e3 * sorted(t_seq)[len(t_seq) // 2] / K,
                         "pyramids_per_pair": T / P},
            "ratio_sequence_over_pair": ss["median"] / ps["median"],
            "rows_bitwise_equal_to_pair_mode": bitwise, "last_window_equal_to_eager_window": last_ok}


def shape4(args, dev):
    from pwclonet_pylidarslam_amd import preprocess
    from pwclonet_pylidarslam_amd.pointnet2_ops import _ext as _ext_mod
    B, rows, npts, near = 8, args.rows, 8192, 35.0
    if args.dry:
        return {"dry": True}
    net = _net(dev, "bf16")
    raw = bench.raw_frames(1, B + 1, rows, dev)                    # one 9-frame window
    raw_pairs = torch.cat((raw[:-1], raw[1:])).contiguous()        # run_config5's layout: 8 frame-1s, then 8 frame-2s
    lib = _lib.load()
    out = {"workload": "BASELINE.json configs[4] shape: %d pairs of raw %d-row frames, KITTI-360 filter, exact sampling "
                       "to %d, bf16 stacks, eager" % (B, rows, npts)}
    for depth in (1, 2):
        order = "torch" if depth > 1 else "device"                # run_config5's choice, on both sides
        _ext_mod.LARGE_CLOUD_ORDER = order
        lib.pwclo_fps_large_cloud_launch(0 if depth > 1 else 1)
        side = [torch.cuda.Stream(device=dev) for _ in range(depth)] if depth > 1 else None
        pyr = torch.cuda.Stream(device=dev) if depth > 1 else None

        def front_pair():
            clouds, _ = preprocess.frames_to_clouds(raw_pairs, npts, dataset="kitti360", near_threshold=near)
            return clouds[:B].transpose(1, 2).contiguous(), clouds[B:].transpose(1, 2).contiguous()

        def back_pair(c):
            with torch.no_grad():
                return net(c[0], None, c[1], None)[0]

        def front_seq():
            return (preprocess.frames_to_clouds(raw, npts, dataset="kitti360", near_threshold=near)[0],)

        def back_seq(c):
            with torch.no_grad():
                return net.forward_sequence(c[0])[0]

        def run(front, back, k):
            if side is None:
                for _ in range(k):
                    o = back(front())
                return o
            main = torch.cuda.current_stream(dev)
            for s_ in side + [pyr]:
                s_.wait_stream(main)
            for i in range(k):                                    # run_config5's split: fronts on two streams, pyramids on a third
                with torch.cuda.stream(side[i % depth]):
                    c = front()
                    ready = torch.cuda.Event()
                    ready.record()
                with torch.cuda.stream(pyr):
                    pyr.wait_event(ready)
                    for t in c:
                        t.record_stream(pyr)
                    o = back(c)
            for s_ in side + [pyr]:
                main.wait_stream(s_)
            return o

        try:
            run(front_pair, back_pair, max(1, args.warmup))
            run(front_seq, back_seq, max(1, args.warmup))
            t_pair, t_seq = [], []
            for _ in range(args.repeats):
                dt, pose_pair = _timed(dev, lambda: run(front_pair, back_pair, args.steps4))
                t_pair.append(dt)
                dt, pose_seq = _timed(dev, lambda: run(front_seq, back_seq, args.steps4))
                t_seq.append(dt)
            _lib.synchronize(dev)                                 # raises if a sampler reported a timeout
        finally:
            lib.pwclo_fps_large_cloud_launch(1)
        ps, ss = _stats(args.steps4 * B, t_pair), _stats(args.steps4 * B, t_seq)
        out["inflight_%d" % depth] = {
            "spatial_order": order, "sampler_launch": "plain" if depth > 1 else "cooperative",
            "pair": {"raw_frames_per_step": 2 * B, "frame_pairs_per_s": ps,
                     "ms_per_step": 1e3 * sorted(t_pair)[len(t_pair) // 2] / args.steps4},
            "sequence": {"raw_frames_per_step": B + 1, "frame_pairs_per_s": ss,
                         "ms_per_step": 1e3 * sorted(t_seq)[len(t_seq) // 2] / args.steps4},
            "ratio_sequence_over_pair": ss["median"] / ps["median"],
            "poses_bitwise_equal": bool(torch.equal(pose_seq, pose_pair))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="configs[2]: windows (= pair batches of 32) per timed region")
    ap.add_argument("--steps4", type=int, default=6, help="configs[4]: steps (8 pairs each) per timed region")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7, help="alternated timed regions per mode")
    ap.add_argument("--inflight", type=int, default=4)
    ap.add_argument("--window", type=int, default=33)
    ap.add_argument("--npoints", type=int, default=8192)
    ap.add_argument("--rows", type=int, default=120000)
    ap.add_argument("--shapes", default="2,4")
    ap.add_argument("--dry", action="store_true", help="host-side set-up only, no device call")
    args = ap.parse_args()
    # before the first HIP call of the process, as bench.py: 4 slots in flight need more than 4 hardware queues
    pwclonet_pylidarslam_amd.configure_hw_queues(8)
    shapes = [int(s) for s in args.shapes.split(",")]
    base = synthetic.kitti_like_sequence(1000, args.npoints, args.window)[0] if 2 in shapes else None
    dev = torch.device("cuda:0")
    if not args.dry:
        torch.cuda.set_device(dev)
        _lib.load()
    out = {"metric": "sequence odometry vs pair mode, frame-pairs/s (median of alternated repeats)",
           "unit": "frame-pairs/s", "repeats": args.repeats, "warmup": args.warmup,
           "hw_queues": pwclonet_pylidarslam_amd.hw_queues()}
    with torch.no_grad():
        if 2 in shapes:
            out["configs2"] = shape2(args, dev, base)
        if 4 in shapes:
            out["configs4"] = shape4(args, dev)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
