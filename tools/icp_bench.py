#!/usr/bin/env python3
"""Time of one point-to-plane registration beside the streaming step, one process; one JSON line.

``IcpRefiner(graph=True)`` at n = 8192, map_size = 4, iters = 10, S = 1 and S = 8: the HIP-event time of one ``register``
replay (one frame in flight: events around the call, a sync after it), median over the frames of a repeat.  Beside it, in
the same process and alternated repeat by repeat, the per-frame time of ``StreamingOdometry(graph=True).step`` at the same
S on the same frames (``tools/stream_bench.py``'s way); median / min / max / spread over ``--repeats`` repeats.  The initial
guess is "no motion" (the identity), 0.5-1.5 m and up to 2 degrees from the truth: the tool's network has random weights,
its pose is no vehicle motion, and a registration that starts there finds no pairs and freezes in iteration 0.  The launch
sequence is fixed either way; what a sensible guess adds is the accumulation over real pairs and the search near the map.

    python tools/icp_bench.py [--frames F] [--repeats R] [--npoints N] [--map-size M] [--iters I]

``--per-stream``: instead, the refiner's two views (one engine, one graph) in the same process,
alternated repeat by repeat: the time of one ``register`` call (its eager loads of cloud, guess and, where given, masks, then
the replay) through the lock-step view, through the per-stream view (``IcpRefiner(per_stream=True)``) with device masks
that say all streams are active and, where there is more than one stream, with every second stream idle; and the two
eager launches ``StreamingOdometry`` adds per call with ``refine=`` (the restart word and ``stream_record_refined``),
timed as a pair over a loop that ends in a sync.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pwclonet_pylidarslam_amd import synthetic  # noqa: E402
from pwclonet_pylidarslam_amd.odometry import StreamingOdometry  # noqa: E402
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet  # noqa: E402
from pwclonet_pylidarslam_amd.registration import IcpRefiner  # noqa: E402


def _stats(xs):
    xs = sorted(xs)
    med = xs[len(xs) // 2]
    return {"median": med, "min": xs[0], "max": xs[-1], "spread_pct": 100.0 * (xs[-1] - xs[0]) / med}


def _per_frame_ms(fn, frames):
    out = []
    for k in range(1, frames):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn(k)
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e))
    return sorted(out)[len(out) // 2]


def _per_stream(a, S, batches, dev):
    """``register`` through the lock-step and the per-stream view on the same frames, alternated; the eager launches of
    the streaming path."""
    from pwclonet_pylidarslam_amd import _lib
    kw = dict(map_size=a.map_size, iters=a.iters, graph=True)
    lock, msk = IcpRefiner(S, a.npoints, **kw), IcpRefiner(S, a.npoints, per_stream=True, **kw)
    eye = torch.eye(4, dtype=torch.float64, device=dev).expand(S, 4, 4).contiguous()
    ones = torch.ones((S,), dtype=torch.int32, device=dev)
    half = torch.tensor([1 - i % 2 for i in range(S)], dtype=torch.int32, device=dev)
    zeros = torch.zeros((S,), dtype=torch.int32, device=dev)

    def lock_pass():
        lock.reset()
        lock.register(batches[0], eye)
        return _per_frame_ms(lambda k: lock.register(batches[k], eye), a.frames)

    def masked_pass(active):
        msk.reset()
        msk.register(batches[0], eye, active=ones, restart=zeros)
        return _per_frame_ms(lambda k: msk.register(batches[k], eye, active=active, restart=zeros), a.frames)

    lock_pass(), lock_pass(), masked_pass(ones), masked_pass(ones), masked_pass(half)      # warm-up and captures
    tl, ta, th = [], [], []
    for _ in range(a.repeats):
        tl.append(lock_pass())
        ta.append(masked_pass(ones))
        if S > 1:
            th.append(masked_pass(half))
    out = {"lockstep_register_ms": _stats(tl), "masked_all_active_register_ms": _stats(ta),
           "masked_over_lockstep": _stats(ta)["median"] / _stats(tl)["median"],
           "launches_per_register": 4 + 4 * a.iters + 1,
           "masked_last_status": msk.status().tolist(), "masked_last_pairs": msk.diagnostics()["pairs"].tolist()}
    if S > 1:
        out["masked_every_second_idle_register_ms"] = _stats(th)
        out["half_idle_over_all_active"] = _stats(th)["median"] / _stats(ta)["median"]
    # the eager launches StreamingOdometry adds per call: restart = active - valid, then the record launch
    cap = 8
    valid, count, restart = ones.clone(), torch.full((S,), 2, dtype=torch.int32, device=dev), zeros.clone()
    rel = torch.zeros((cap, S, 4, 4), dtype=torch.float64, device=dev)
    ab = torch.eye(4, dtype=torch.float64, device=dev).expand(cap, S, 4, 4).contiguous()
    T = msk.bufs["T"]

    def extra():
        torch.sub(ones, valid, out=restart)
        _lib.call("stream_record_refined_kernel_wrapper", dev, S, cap, ones.data_ptr(), valid.data_ptr(), count.data_ptr(),
                  T.data_ptr(), rel.data_ptr(), ab.data_ptr())

    loops, te = 200, []
    for _ in range(20):
        extra()
    for _ in range(a.repeats):
        torch.cuda.synchronize(dev)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(loops):
            extra()
        e.record()
        e.synchronize()
        te.append(1000.0 * s.elapsed_time(e) / loops)
    out["streaming_extra_eager_us_per_call"] = _stats(te)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=41)
    ap.add_argument("--base", type=int, default=21, help="frames generated; the streams bounce through them")
    ap.add_argument("--npoints", type=int, default=8192)
    ap.add_argument("--map-size", type=int, default=4)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--per-stream", action="store_true", help="the masked refiner beside the lock-step one")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    base = torch.from_numpy(synthetic.kitti_like_sequence(2024, a.npoints, a.base)[0]).to(dev)[:, :, :3].contiguous()
    period = 2 * (a.base - 1)
    order = [min(k % period, period - k % period) for k in range(a.frames + 40)]
    torch.manual_seed(1234)
    net = PWCLONet(dict(num_input_channels=3, sequence_len=2, device=str(dev), scalar_last=False, log_mode="none"))
    net = net.to(dev).eval().prepare_fused()
    res = {"tool": "icp_bench", "npoints": a.npoints, "map_size": a.map_size, "iters": a.iters, "frames": a.frames,
           "repeats": a.repeats, "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES")}
    if a.per_stream:
        res["mode"] = "per_stream"
        for S in (1, 8):
            batches = [base[torch.tensor([order[k + 5 * i] for i in range(S)], device=dev)] for k in range(a.frames)]
            res["s%d" % S] = _per_stream(a, S, batches, dev)
        print(json.dumps(res))
        return
    for S in (1, 8):
        batches = [base[torch.tensor([order[k + 5 * i] for i in range(S)], device=dev)] for k in range(a.frames)]
        so = StreamingOdometry(net, streams=S, max_frames=a.frames + 1, graph=True)
        ref = IcpRefiner(S, a.npoints, map_size=a.map_size, iters=a.iters, graph=True)
        eye = torch.eye(4, dtype=torch.float64, device=dev).expand(S, 4, 4).contiguous()

        def stream_pass():
            so.reset()
            so.step(batches[0])
            return _per_frame_ms(lambda k: so.step(batches[k]), a.frames)

        def icp_pass():
            ref.reset()
            ref.register(batches[0], eye)
            return _per_frame_ms(lambda k: ref.register(batches[k], eye), a.frames)

        stream_pass(), icp_pass(), icp_pass()                                 # warm-up; the second icp pass replays only
        ts, ti = [], []
        for _ in range(a.repeats):
            ts.append(stream_pass())
            ti.append(icp_pass())
        d = ref.diagnostics()
        res["s%d" % S] = {"register_ms": _stats(ti), "stream_step_ms": _stats(ts),
                          "register_over_step": _stats(ti)["median"] / _stats(ts)["median"],
                          "launches_per_register": 4 + 4 * a.iters + 1,
                          "last_status": ref.status().tolist(), "last_pairs": d["pairs"].tolist(),
                          "last_iterations": d["iterations"].tolist()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
