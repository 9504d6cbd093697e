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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=41)
    ap.add_argument("--base", type=int, default=21, help="frames generated; the streams bounce through them")
    ap.add_argument("--npoints", type=int, default=8192)
    ap.add_argument("--map-size", type=int, default=4)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
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
                          "launches_per_register": 3 + 4 * a.iters + 1,
                          "last_status": ref.status().tolist(), "last_pairs": d["pairs"].tolist(),
                          "last_iterations": d["iterations"].tolist()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
