#!/usr/bin/env python3
"""Streaming odometry from raw sweeps against pair mode on raw frames, one process, alternated and repeated; one JSON line.

Input: ``synthetic.raw_sweep_sequence`` sweeps (64 x 2048 rays, ~118-127k rows each, every length different), KITTI-360
front end (near 30 m), capacity 131072, 8192 points.  A long stream plays one generated sequence forwards and backwards.
(a) S = 1, one frame in flight, HIP events around each call and a sync after it: per-frame time of
    ``StreamingOdometry(graph=True, sweeps=...).step_sweeps`` (filter + compaction + sampler + pyramid + pair stage in
    the captured graphs) against pair mode on the raw frames: ``frames_to_clouds`` of the previous and of the new sweep
    (eager: the row counts differ, so the two cannot share one call) + ``GraphedForward`` at batch 1.
(b) S = 8 (streams start at different frames): frames/s of ``step_sweeps`` against pair mode (16 ``frames_to_clouds``
    calls + ``GraphedForward`` at batch 8), one step in flight, HIP events around a region of back-to-back steps.
(c) ``sweep_filter_compact_kernel`` alone (HIP events around 50 back-to-back launches) at S = 1 and S = 8.
Modes alternate repeat by repeat; medians over frames per repeat, then median / spread over repeats.
Check: the streamed rows equal pair mode's bit for bit (the pair forward is the streaming contract's reference).
(d) ``--voxel-size V [--voxel-capacity C]``: the grid-sampled front end against the plain one, in
    this process and alternated repeat by repeat: kept rows and voxel winners per generated sweep (at V and at 0.1 .. 0.5 m),
    ``sweep_filter_grid_compact_kernel`` against ``sweep_filter_compact_kernel`` alone, S = 1 ms per frame and S = 8
    frames/s of ``step_sweeps`` without a grid, with the grid at ``voxel_capacity = capacity``, and with
    ``voxel_capacity = C``.

(e) ``--deskew``: the de-skewing front end against the plain one, in this process and alternated
    repeat by repeat, with synthetic times proportional to the row index: S = 1 ms per frame and S = 8 frames/s of
    ``step_sweeps`` with ``deskew`` off and on, and ``sweep_filter_deskew_compact_kernel`` against
    ``sweep_filter_compact_kernel`` alone under HIP events, on the sweeps and the motion loaded last.

    python tools/raw_stream_bench.py [--frames F] [--repeats R] [--steps8 K] [--voxel-size V [--voxel-capacity C]] [--deskew]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pwclonet_pylidarslam_amd import _lib, preprocess, synthetic  # noqa: E402
from pwclonet_pylidarslam_amd.graphed import GraphedForward  # noqa: E402
from pwclonet_pylidarslam_amd.odometry import StreamingOdometry  # noqa: E402
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet  # noqa: E402

CAP, NPOINTS, NEAR = 131072, 8192, 30.0


def _stats(xs):
    xs = sorted(xs)
    med = xs[len(xs) // 2]
    return {"median": med, "min": xs[0], "max": xs[-1], "spread_pct": 100.0 * (xs[-1] - xs[0]) / med}


def _ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=41, help="frames of the S = 1 stream")
    ap.add_argument("--base", type=int, default=12, help="sweeps generated; the streams bounce through them")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps8", type=int, default=10, help="steps per timed region at S = 8")
    ap.add_argument("--voxel-size", type=float, default=None, help="also measure the grid-sampled front end at this size")
    ap.add_argument("--voxel-capacity", type=int, default=None, help="with --voxel-size: a packed width to measure as well")
    ap.add_argument("--deskew", action="store_true", help="also measure the de-skewing front end against the plain one")
    a = ap.parse_args()
    if a.voxel_capacity is not None and a.voxel_size is None:
        ap.error("--voxel-capacity needs --voxel-size")
    dev = torch.device("cuda:0")
    base = [torch.from_numpy(s).to(dev) for s in synthetic.raw_sweep_sequence(2024, a.base)[0]]
    period = 2 * (a.base - 1)
    order = [min(k % period, period - k % period) for k in range(max(a.frames, a.steps8 + 8 * 3 + 1))]
    torch.manual_seed(1234)
    net = PWCLONet(dict(num_input_channels=3, sequence_len=2, device=str(dev), scalar_last=False,
                        log_mode="none")).to(dev).eval().prepare_fused()
    torch.set_grad_enabled(False)
    sweeps_cfg = dict(dataset="kitti360", capacity=CAP, near_threshold=NEAR)
    res = {"tool": "raw_stream_bench", "capacity": CAP, "npoints": NPOINTS, "frames": a.frames, "repeats": a.repeats,
           "rows": [int(s.shape[0]) for s in base], "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES")}

    def cloud(k):
        sw = base[order[k]]
        return preprocess.frames_to_clouds(sw[None], NPOINTS, "kitti360", near_threshold=NEAR, cap=CAP)[0]

    def cm(c):
        return c.permute(0, 2, 1).contiguous()

    # ---- (a) S = 1 ----
    so = StreamingOdometry(net, streams=1, max_frames=a.frames + 1, graph=True, sweeps=sweeps_cfg)
    pair = GraphedForward(net)

    def stream_frame(k):
        sw = base[order[k]]
        return so.step_sweeps(sw[None], [sw.shape[0]])

    def pair_frame(k):
        return pair(cm(cloud(k - 1)), cm(cloud(k)))

    def stream_pass():
        so.reset()
        stream_frame(0)
        return sorted(_ms(lambda: stream_frame(k))[0] for k in range(1, a.frames))[(a.frames - 1) // 2]

    def pair_pass():
        return sorted(_ms(lambda: pair_frame(k))[0] for k in range(1, a.frames))[(a.frames - 1) // 2]

    so.reset()
    stream_frame(0)
    same = all(torch.equal(stream_frame(k), pair_frame(k)) for k in range(1, min(a.frames, 8)))
    stream_pass(), pair_pass()                                            # warm-up
    ts, tp = [], []
    for _ in range(a.repeats):
        ts.append(stream_pass())
        tp.append(pair_pass())
    res["s1_raw_stream_ms_per_frame"] = _stats(ts)
    res["s1_raw_pair_ms_per_frame"] = _stats(tp)
    res["s1_latency_ratio_pair_over_stream"] = _stats(tp)["median"] / _stats(ts)["median"]
    res["s1_rows_bitwise_equal_pair"] = bool(same)

    # ---- (b) S = 8 ----
    S = 8
    idx = [[k + 3 * i for i in range(S)] for k in range(a.steps8 + 1)]    # stream i starts 3 i frames later
    so8 = StreamingOdometry(net, streams=S, max_frames=a.steps8 + 2, graph=True, sweeps=sweeps_cfg)
    pair8 = GraphedForward(net)

    def batch(k):
        rows = [base[order[j]] for j in idx[k]]
        lengths = [int(r.shape[0]) for r in rows]
        out = torch.zeros((S, max(lengths), 4), dtype=torch.float32, device=dev)
        for s, r in enumerate(rows):
            out[s, :r.shape[0]] = r
        return out, lengths

    batches = [batch(k) for k in range(a.steps8 + 1)]

    def clouds8(k):
        return torch.cat([cloud(j) for j in idx[k]])

    def stream8():
        so8.reset()
        so8.step_sweeps(*batches[0])
        return _ms(lambda: [so8.step_sweeps(*batches[k]) for k in range(1, a.steps8 + 1)])[0]

    def pair8_pass():
        return _ms(lambda: [pair8(cm(clouds8(k - 1)), cm(clouds8(k))) for k in range(1, a.steps8 + 1)])[0]

    so8.reset()
    so8.step_sweeps(*batches[0])
    same8 = all(torch.equal(so8.step_sweeps(*batches[k]), pair8(cm(clouds8(k - 1)), cm(clouds8(k)))) for k in (1, 2))
    stream8(), pair8_pass()
    r_s, r_p = [], []
    for _ in range(a.repeats):
        r_s.append(S * a.steps8 / (stream8() / 1e3))
        r_p.append(S * a.steps8 / (pair8_pass() / 1e3))
    res["s8_raw_stream_frames_per_s"] = _stats(r_s)
    res["s8_raw_pair_pairs_per_s"] = _stats(r_p)
    res["s8_ratio_stream_over_pair"] = _stats(r_s)["median"] / _stats(r_p)["median"]
    res["s8_rows_bitwise_equal_pair"] = bool(same8)

    # ---- (c) the filter + compaction kernel alone ----
    for name, front in (("s1", so._front), ("s8", so8._front)):
        b = front.bufs

        def launches():
            for _ in range(50):
                _lib.call("sweep_filter_compact_kernel_wrapper", dev, front.streams, CAP, CAP, b["lengths"].data_ptr(),
                          b["sweeps"].data_ptr(), 1, 0, front.ground_z, front.near_threshold, b["packed"].data_ptr(),
                          b["counts"].data_ptr())
        launches()
        res["sweep_filter_compact_ms_" + name] = _stats([_ms(launches)[0] / 50 for _ in range(5)])
    if a.voxel_size is not None:
        _grid_section(a, res, dev, net, base, order, batches, so, so8)
    if a.deskew:
        _deskew_section(a, res, dev, net, base, order, batches, so, so8)
    res["sampler_workgroups_per_pose"] = {"stream": -(-CAP // 16384), "pair": 2 * -(-CAP // 16384)}
    torch.cuda.synchronize(dev)
    res["last_error"] = int(_lib.load().pwclo_last_error())
    print(json.dumps(res))


def _grid_section(a, res, dev, net, base, order, batches, so, so8):
    """Section (d): the plain front end (``so`` / ``so8``, already warm) against the grid-sampled one, alternated."""
    V, S = a.voxel_size, 8
    widths = [CAP] + ([a.voxel_capacity] if a.voxel_capacity is not None else [])
    cfg = dict(dataset="kitti360", capacity=CAP, near_threshold=NEAR, voxel_size=V)
    # kept rows and winners of every generated sweep (the synthetic scene: planes, not real LiDAR)
    sizes = sorted({V, 0.1, 0.2, 0.3, 0.5})
    winners = {"%g" % v: [] for v in sizes}
    kept = []
    for sw in base:
        xyz, keep = preprocess.kitti360_filter(sw[None], NEAR)
        kept.append(int(keep.sum()))
        for v in sizes:
            winners["%g" % v].append(int(preprocess.grid_sample(xyz, v, keep=keep)[1][0]))
    res["voxel_size"], res["voxel_capacity"] = V, a.voxel_capacity
    res["kept_rows_per_sweep"] = kept
    res["voxel_winners_per_sweep"] = winners

    def s1_pass(obj):
        obj.reset()
        obj.step_sweeps(base[order[0]][None], [base[order[0]].shape[0]])
        ts = [_ms(lambda: obj.step_sweeps(base[order[k]][None], [base[order[k]].shape[0]]))[0] for k in range(1, a.frames)]
        return sorted(ts)[len(ts) // 2]

    def s8_pass(obj):
        obj.reset()
        obj.step_sweeps(*batches[0])
        t = _ms(lambda: [obj.step_sweeps(*batches[k]) for k in range(1, a.steps8 + 1)])[0]
        return S * a.steps8 / (t / 1e3)

    one = {"none": so}
    eight = {"none": so8}
    for w in widths:
        one["width_%d" % w] = StreamingOdometry(net, streams=1, max_frames=a.frames + 1, graph=True,
                                                sweeps=dict(cfg, voxel_capacity=w))
        eight["width_%d" % w] = StreamingOdometry(net, streams=S, max_frames=a.steps8 + 2, graph=True,
                                                  sweeps=dict(cfg, voxel_capacity=w))
    t1 = {k: [] for k in one}
    t8 = {k: [] for k in eight}
    for k in one:                                                             # warm-up and capture
        s1_pass(one[k]), s8_pass(eight[k])
    for _ in range(a.repeats):
        for k in one:
            t1[k].append(s1_pass(one[k]))
        for k in eight:
            t8[k].append(s8_pass(eight[k]))
    res["grid_s1_ms_per_frame"] = {k: _stats(v) for k, v in t1.items()}
    res["grid_s8_frames_per_s"] = {k: _stats(v) for k, v in t8.items()}
    res["grid_s1_overflowed"] = {k: bool((one[k].voxel_counts() > one[k]._front.width).any()) for k in one if k != "none"}

    # the first launch alone: filter + compaction against filter + grid + compaction, on the sweeps loaded last
    tk = {}
    for name, plain, grid in (("s1", so._front, one["width_%d" % CAP]._front), ("s8", so8._front, eight["width_%d" % CAP]._front)):
        b, g = plain.bufs, grid.bufs

        def old():
            for _ in range(50):
                _lib.call("sweep_filter_compact_kernel_wrapper", dev, plain.streams, CAP, CAP, b["lengths"].data_ptr(),
                          b["sweeps"].data_ptr(), 1, 0, plain.ground_z, plain.near_threshold, b["packed"].data_ptr(),
                          b["counts"].data_ptr())

        def new():
            for _ in range(50):
                _lib.call("sweep_filter_grid_compact_kernel_wrapper", dev, grid.streams, CAP, CAP, g["lengths"].data_ptr(),
                          g["sweeps"].data_ptr(), 1, 0, grid.ground_z, grid.near_threshold, V, g["grid_ws"].data_ptr(),
                          g["packed"].data_ptr(), g["counts"].data_ptr(), g["winners"].data_ptr())
        old(), new()
        t_old, t_new = [], []
        for _ in range(a.repeats):
            t_old.append(_ms(old)[0] / 50)
            t_new.append(_ms(new)[0] / 50)
        tk[name] = {"sweep_filter_compact_ms": _stats(t_old), "sweep_filter_grid_compact_ms": _stats(t_new),
                    "rows": g["lengths"].tolist(), "winners": g["winners"].tolist()}
    res["grid_first_launch"] = tk


def _deskew_section(a, res, dev, net, base, order, batches, so, so8):
    """Section (e): the plain front end (``so`` / ``so8``, already warm) against the de-skewing one, alternated."""
    S = 8
    cfg = dict(dataset="kitti360", capacity=CAP, near_threshold=NEAR, deskew=True)

    def times(shape):                                                         # 0.1 s per sweep, proportional to the row index
        return (0.1 * torch.arange(shape[1], dtype=torch.float64, device=dev) / shape[1]).expand(shape[0], -1).contiguous()

    t1 = [times((1, sw.shape[0])) for sw in base]
    t8 = [times(b[0].shape[:2]) for b in batches]
    one = {"off": so, "on": StreamingOdometry(net, streams=1, max_frames=a.frames + 1, graph=True, sweeps=cfg)}
    eight = {"off": so8, "on": StreamingOdometry(net, streams=S, max_frames=a.steps8 + 2, graph=True, sweeps=cfg)}

    def step1(key, k):
        sw = base[order[k]]
        kw = dict(times=t1[order[k]]) if key == "on" else {}
        return one[key].step_sweeps(sw[None], [sw.shape[0]], **kw)

    def step8(key, k):
        kw = dict(times=t8[k]) if key == "on" else {}
        return eight[key].step_sweeps(*batches[k], **kw)

    def s1_pass(key):
        one[key].reset()
        step1(key, 0)
        ts = [_ms(lambda: step1(key, k))[0] for k in range(1, a.frames)]
        return sorted(ts)[len(ts) // 2]

    def s8_pass(key):
        eight[key].reset()
        step8(key, 0)
        t = _ms(lambda: [step8(key, k) for k in range(1, a.steps8 + 1)])[0]
        return S * a.steps8 / (t / 1e3)

    r1 = {k: [] for k in one}
    r8 = {k: [] for k in eight}
    for k in one:                                                             # warm-up and capture
        s1_pass(k), s8_pass(k)
    for _ in range(a.repeats):
        for k in one:
            r1[k].append(s1_pass(k))
        for k in eight:
            r8[k].append(s8_pass(k))
    res["deskew_s1_ms_per_frame"] = {k: _stats(v) for k, v in r1.items()}
    res["deskew_s8_frames_per_s"] = {k: _stats(v) for k, v in r8.items()}
    res["deskew_motion_s1"] = one["on"].motion()[0].tolist()

    # the first launch alone: filter + compaction against filter + de-skew + compaction, on the sweeps loaded last
    tk = {}
    for name, plain, desk in (("s1", so._front, one["on"]._front), ("s8", so8._front, eight["on"]._front)):
        b, g = plain.bufs, desk.bufs

        def old():
            for _ in range(50):
                _lib.call("sweep_filter_compact_kernel_wrapper", dev, plain.streams, CAP, CAP, b["lengths"].data_ptr(),
                          b["sweeps"].data_ptr(), 1, 0, plain.ground_z, plain.near_threshold, b["packed"].data_ptr(),
                          b["counts"].data_ptr())

        def new():
            for _ in range(50):
                _lib.call("sweep_filter_deskew_compact_kernel_wrapper", dev, desk.streams, CAP, CAP, g["lengths"].data_ptr(),
                          g["sweeps"].data_ptr(), 1, 0, desk.ground_z, desk.near_threshold, g["times"].data_ptr(),
                          g["motion"].data_ptr(), 0, 0, g["packed"].data_ptr(), g["counts"].data_ptr())
        old(), new()
        t_old, t_new = [], []
        for _ in range(a.repeats):
            t_old.append(_ms(old)[0] / 50)
            t_new.append(_ms(new)[0] / 50)
        tk[name] = {"sweep_filter_compact_ms": _stats(t_old), "sweep_filter_deskew_compact_ms": _stats(t_new),
                    "rows": g["lengths"].tolist(), "kept": g["counts"].tolist()}
    res["deskew_first_launch"] = tk


if __name__ == "__main__":
    main()
