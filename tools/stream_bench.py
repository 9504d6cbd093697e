#!/usr/bin/env python3
"""Streaming odometry against pair mode, one process, alternated and repeated; prints one JSON line.

(a) S = 1, 8192 points: per-frame time of ``StreamingOdometry(graph=True)`` against ``GraphedForward`` at batch 1 on
    the same consecutive pairs: ``--frames`` frames that go forwards and backwards through one
    ``synthetic.kitti_like_sequence`` of ``--base`` frames.  Each frame is timed on its own with HIP
    events around the call and a sync after it (a live sensor: one frame in flight); a repeat = all frames of the
    sequence, the two modes alternate repeat by repeat; median over frames per repeat, then median / spread over
    repeats.  Also: the serial GPU time of one eager step / pair forward (sum of per-launch HIP events).
(b) S = 32: frames/s of ``StreamingOdometry(graph=True)`` against ``GraphedForward`` at batch 32 (the same 32 pairs per
    step), one in flight (HIP events around a region of back-to-back steps), alternated, repeated.
(c) launches per step (eager, ``_lib`` launch sites; the pair forward's for comparison) and the handover: the bytes the
    captured step moves into the persistent previous frame and the time of that one launch alone (eager, HIP events).
Check: the streamed rows equal the pair forward's at the same batch bit for bit.

    python tools/stream_bench.py [--frames F] [--repeats R] [--steps32 K] [--trace-only] [--per-stream]

``--trace-only``: only the S = 1 graphed stream over the frames, for ``rocprofv3 --kernel-trace --stats -- python
tools/stream_bench.py --trace-only`` (a run of its own).

``--per-stream``: instead of (a)-(c), ``StreamingOdometry(per_stream=True)`` beside the lock-step
object, alternated repeat by repeat in this process: S = 1 per-frame time (all active), S = 32 frames/s with all streams
active and with every other stream active (steps x S per second in both: an idle stream costs what an active one does).
With all streams active the two objects replay the SAME graph (the same launches) through two front doors, so the
``lockstep`` / ``masked`` all-active pair measures the host front ends and the run's noise, not two kernels; the
half-active series is the one only per-stream mode can run.  At S = 32 also the masked handover launch alone against one
``copy_`` per tensor, which is what the step did before it had the launch (HIP events, bytes read + written per
second).  ``--per-stream --trace-only``: only 30 masked handover launches at S = 32, all streams
active, for ``rocprofv3 --kernel-trace --stats -- python tools/stream_bench.py --per-stream --trace-only`` (a run of its own):
the kernel's device time without launch latency.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pwclonet_pylidarslam_amd import _lib, synthetic  # noqa: E402
from pwclonet_pylidarslam_amd.graphed import GraphedForward  # noqa: E402
from pwclonet_pylidarslam_amd.odometry import StreamingOdometry  # noqa: E402
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet  # noqa: E402


def _net(dev):
    torch.manual_seed(1234)
    net = PWCLONet(dict(num_input_channels=3, sequence_len=2, device=str(dev), scalar_last=False,
                        log_mode="none")).to(dev).eval()
    return net.prepare_fused()


def _cm(frames):
    return frames[:, :, :3].permute(0, 2, 1).contiguous()


def _stats(xs):
    xs = sorted(xs)
    med = xs[len(xs) // 2]
    return {"median": med, "min": xs[0], "max": xs[-1], "spread_pct": 100.0 * (xs[-1] - xs[0]) / med}


class _Rec:
    def __init__(self):
        self.rows = []

    def add(self, name, meta, s, e):
        self.rows.append((name, s, e))


def _launches(dev, fn):
    """(launch sites, serial GPU ms) of one eager call."""
    rec = _Rec()
    _lib.profiler = rec
    try:
        fn()
    finally:
        _lib.profiler = None
    torch.cuda.synchronize(dev)
    return len(rec.rows), sum(s.elapsed_time(e) for _, s, e in rec.rows)


def _per_frame_ms(dev, fn, frames):
    """Median over frames of the HIP-event time of fn(k), one frame in flight."""
    out = []
    for k in range(1, frames):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn(k)
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e))
    return sorted(out)[len(out) // 2]


def _region_ms(dev, fn, steps):
    torch.cuda.synchronize(dev)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for k in range(steps):
        fn(k)
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def _per_stream(a, dev, net, clouds, res):
    """``--per-stream``: the per-stream front door against the lock-step one (all active: the same graph), same
    frames, alternated; then the series with every other stream active."""
    F = a.frames
    if a.trace_only:
        S = 32
        fs = net._fused
        batch = clouds[torch.tensor([(5 * i) % F for i in range(S)], device=dev)]
        new = fs.stream_prime(batch, a.npoints)
        slot = new.frame1_buffers()
        ones = torch.ones((S,), dtype=torch.int32, device=dev)
        for _ in range(30):
            slot.copy_frame1_masked_(new, ones)
        torch.cuda.synchronize(dev)
        print(json.dumps({"tool": "stream_bench", "mode": "per_stream", "trace_only": True, "launches": 30,
                          "bytes": slot.frame1_bytes()}))
        return
    lock = StreamingOdometry(net, streams=1, max_frames=F + 1, graph=True)
    per = StreamingOdometry(net, streams=1, max_frames=F + 1, graph=True, per_stream=True)

    def run1(so):
        so.reset()
        so.step(clouds[0:1])
        return _per_frame_ms(dev, lambda k: so.step(clouds[k:k + 1]), F)

    lock.reset(), per.reset()
    lock.step(clouds[0:1]), per.step(clouds[0:1])
    same = all(torch.equal(per.step(clouds[k:k + 1]), lock.step(clouds[k:k + 1])) for k in range(1, min(F, 20)))
    run1(lock), run1(per)
    tl, tm = [], []
    for _ in range(a.repeats):
        tl.append(run1(lock))
        tm.append(run1(per))
    res["s1_lockstep_ms_per_frame"], res["s1_masked_ms_per_frame"] = _stats(tl), _stats(tm)
    res["s1_rows_bitwise_equal_lockstep"] = bool(same)
    res["all_active_note"] = ("lockstep and masked all-active are the same captured launches entered through "
                              "step(frames) and step(frames, active=None) of two objects")

    S, K = 32, a.steps32
    idx = [[(k + 5 * i) % F for i in range(S)] for k in range(K + 1)]
    batches = [clouds[torch.tensor(r, device=dev)] for r in idx]
    lock32 = StreamingOdometry(net, streams=S, max_frames=K + 2, graph=True)
    per32 = StreamingOdometry(net, streams=S, max_frames=K + 2, graph=True, per_stream=True)
    half = torch.tensor([i % 2 == 0 for i in range(S)], device=dev)

    def run32(so, mask=None):
        so.reset()
        so.step(batches[0])
        step = (lambda k: so.step(batches[k + 1])) if mask is None else (lambda k: so.step(batches[k + 1], active=mask))
        return S * K / (_region_ms(dev, step, K) / 1e3)

    lock32.reset(), per32.reset()
    lock32.step(batches[0]), per32.step(batches[0])
    same32 = all(torch.equal(per32.step(batches[k]), lock32.step(batches[k])) for k in range(1, 4))
    run32(lock32), run32(per32), run32(per32, half)
    rl, ra, rh = [], [], []
    for _ in range(a.repeats):
        rl.append(run32(lock32))
        ra.append(run32(per32))
        rh.append(run32(per32, half))
    res["s32_lockstep_frames_per_s"] = _stats(rl)
    res["s32_masked_all_active_frames_per_s"] = _stats(ra)
    res["s32_masked_half_active_stream_steps_per_s"] = _stats(rh)
    res["s32_rows_bitwise_equal_lockstep"] = bool(same32)

    # the handover alone at S = 32: one masked launch (all active, half active) against one copy_ per tensor
    fs = net._fused
    prev = fs.stream_prime(batches[0], a.npoints)
    _, new = fs.stream_step(prev, batches[1], a.npoints)
    slot = new.frame1_buffers()
    ones = torch.ones((S,), dtype=torch.int32, device=dev)
    halfi = half.to(torch.int32)

    def timed(fn):
        out = []
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        for _ in range(30):
            s.record()
            fn()
            e.record()
            e.synchronize()
            out.append(s.elapsed_time(e))
        return _stats(out[5:])

    nbytes = slot.frame1_bytes()
    t_copy, t_all, t_half = (timed(lambda: slot.copy_frame1_(new)), timed(lambda: slot.copy_frame1_masked_(new, ones)),
                             timed(lambda: slot.copy_frame1_masked_(new, halfi)))
    res["handover_s32"] = {"bytes": nbytes, "segments": len(new.frame1_segments(slot)),
                           "copies_lockstep": len(slot.frame1_tensors()), "lockstep_copies_ms": t_copy,
                           "masked_all_active_ms": t_all, "masked_half_active_ms": t_half,
                           "masked_all_active_read_plus_write_TBps": 2.0 * nbytes / (t_all["median"] * 1e-3) / 1e12,
                           "masked_half_active_read_plus_write_TBps": nbytes / (t_half["median"] * 1e-3) / 1e12}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=201, help="frames of the S = 1 sequence (pairs = frames - 1)")
    ap.add_argument("--npoints", type=int, default=8192)
    ap.add_argument("--base", type=int, default=26, help="frames generated; the stream bounces through them")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps32", type=int, default=20, help="steps per timed region at S = 32")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--per-stream", action="store_true", help="the per-stream front door beside the lock-step one, and half-active streams (section 18)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    base = torch.from_numpy(synthetic.kitti_like_sequence(2024, a.npoints, a.base)[0]).to(dev)   # (base, N, 4)
    # a long stream from one generated sequence played forwards and backwards: every pair is a real consecutive pair
    # (the generator's cost grows faster than linearly with the sequence length)
    period = 2 * (a.base - 1)
    seq = base[torch.tensor([min(k % period, period - k % period) for k in range(a.frames)], device=dev)]
    clouds = seq[:, :, :3].contiguous()                                                           # (F, N, 3)
    net = _net(dev)
    res = {"tool": "stream_bench", "npoints": a.npoints, "frames": a.frames, "base": a.base, "repeats": a.repeats,
           "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES")}
    torch.set_grad_enabled(False)
    if a.per_stream:
        res["mode"] = "per_stream"
        return _per_stream(a, dev, net, clouds, res)

    # ---- (a) S = 1 ----
    so = StreamingOdometry(net, streams=1, max_frames=a.frames + 1, graph=True)
    pair = GraphedForward(net)
    x1 = [_cm(seq[k - 1:k]) for k in range(1, a.frames)]
    x2 = [_cm(seq[k:k + 1]) for k in range(1, a.frames)]

    def stream_pass():
        so.reset()
        so.step(clouds[0:1])
        return _per_frame_ms(dev, lambda k: so.step(clouds[k:k + 1]), a.frames)

    if a.trace_only:
        stream_pass()
        torch.cuda.synchronize(dev)
        print(json.dumps({"tool": "stream_bench", "trace_only": True, "frames": a.frames}))
        return
    pair_pass = lambda: _per_frame_ms(dev, lambda k: pair(x1[k - 1], x2[k - 1]), a.frames)
    # check: every streamed row of the sequence is the graphed pair forward's at batch 1
    so.reset()
    so.step(clouds[0:1])
    same = True
    for k in range(1, a.frames):
        same &= torch.equal(so.step(clouds[k:k + 1]), pair(x1[k - 1], x2[k - 1]))
    stream_pass(), pair_pass()                                            # warm-up
    ts, tp = [], []
    for _ in range(a.repeats):
        ts.append(stream_pass())
        tp.append(pair_pass())
    res["s1_stream_ms_per_frame"] = _stats(ts)
    res["s1_pair_ms_per_frame"] = _stats(tp)
    res["s1_latency_ratio_pair_over_stream"] = res["s1_pair_ms_per_frame"]["median"] / res["s1_stream_ms_per_frame"]["median"]
    res["s1_rows_bitwise_equal_pair_b1"] = bool(same)
    fs = net._fused
    prev = fs.stream_prime(clouds[0:1], a.npoints)
    n_stream, gpu_stream = _launches(dev, lambda: fs.stream_step(prev, clouds[1:2], a.npoints))
    n_pair, gpu_pair = _launches(dev, lambda: fs(x1[0], x2[0]))
    res["s1_serial_gpu_ms"] = {"stream_step": gpu_stream, "pair_b1": gpu_pair}

    # ---- (c) launches and handover ----
    _, new = fs.stream_step(prev, clouds[1:2], a.npoints)
    slot = new.frame1_buffers()
    one = torch.ones((1,), dtype=torch.int32, device=dev)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    times = []
    for _ in range(20):
        s.record()
        slot.copy_frame1_masked_(new, one)
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e))
    res["launches_per_step"] = {"stream_step_eager": n_stream, "append": 1, "handover_launches": 1,
                                "handover_segments": len(new.frame1_segments(slot)),
                                "pair_forward_eager": n_pair}
    res["handover"] = {"bytes_s1": so.handover_bytes, "launch_ms_s1": _stats(times)}

    # ---- (b) S = 32 ----
    S = 32
    idx = [[(k + 5 * i) % a.frames for i in range(S)] for k in range(a.steps32 + 1)]   # stream i starts at frame 5 i
    batches = [clouds[torch.tensor(r, device=dev)] for r in idx]                      # (S, N, 3) per step
    so32 = StreamingOdometry(net, streams=S, max_frames=a.steps32 + 2, graph=True)
    pair32 = GraphedForward(net)
    p1 = [_cm(batches[k - 1]) for k in range(1, a.steps32 + 1)]
    p2 = [_cm(batches[k]) for k in range(1, a.steps32 + 1)]

    def stream32():
        so32.reset()
        so32.step(batches[0])
        return _region_ms(dev, lambda k: so32.step(batches[k + 1]), a.steps32)

    pair32_pass = lambda: _region_ms(dev, lambda k: pair32(p1[k], p2[k]), a.steps32)
    so32.reset()
    so32.step(batches[0])
    same32 = all(torch.equal(so32.step(batches[k]), pair32(p1[k - 1], p2[k - 1])) for k in range(1, 4))
    stream32(), pair32_pass()
    r_s, r_p = [], []
    for _ in range(a.repeats):
        r_s.append(S * a.steps32 / (stream32() / 1e3))
        r_p.append(S * a.steps32 / (pair32_pass() / 1e3))
    res["s32_stream_frames_per_s"] = _stats(r_s)
    res["s32_pair_pairs_per_s"] = _stats(r_p)
    res["s32_ratio_stream_over_pair"] = res["s32_stream_frames_per_s"]["median"] / res["s32_pair_pairs_per_s"]["median"]
    res["s32_rows_bitwise_equal_pair_b32"] = bool(same32)
    res["handover"]["bytes_s32"] = so32.handover_bytes
    prev32 = fs.stream_prime(batches[0], a.npoints)
    res["s32_serial_gpu_ms"] = {"stream_step": _launches(dev, lambda: fs.stream_step(prev32, batches[1], a.npoints))[1],
                                "pair_b32": _launches(dev, lambda: fs(p1[0], p2[0]))[1]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
