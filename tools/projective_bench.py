#!/usr/bin/env python3
"""Time of one projective registration beside the knn refiner's (section 21), one process; one JSON
line.

``ProjectiveIcpRefiner(graph=True)`` at 64 x 1800 from 120 000-row sweeps (``synthetic.raw_sweep_sequence``, xyz only),
map_size = 4, iters = 10, S = 1 and S = 8: the HIP-event time of one ``register`` call (its eager loads of rows, lengths and
guess, then the replay; one frame in flight: events around the call, a sync after it), median over the frames of a repeat.
Beside it, in the same process and alternated repeat by repeat, ``IcpRefiner(graph=True).register`` at n = 8192 on
``synthetic.kitti_like_sequence`` clouds, as ``tools/icp_bench.py`` times it; median / min / max / spread over ``--repeats``
repeats.  The initial guess is "no motion" (the identity) on both sides.  The two sides register different inputs (every
kept row of a sweep against 8192 sampled points), so the figures stand beside each other; they are not one workload.

    python tools/projective_bench.py [--frames F] [--repeats R] [--rows N] [--height H] [--width W] [--map-size M] [--iters I]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pwclonet_pylidarslam_amd import synthetic  # noqa: E402
from pwclonet_pylidarslam_amd.projective import ProjectiveIcpRefiner  # noqa: E402
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
    ap.add_argument("--frames", type=int, default=21)
    ap.add_argument("--base", type=int, default=6, help="sweeps generated; the streams bounce through them")
    ap.add_argument("--rows", type=int, default=120000)
    ap.add_argument("--npoints", type=int, default=8192)
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--width", type=int, default=1800)
    ap.add_argument("--map-size", type=int, default=4)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    raw = synthetic.raw_sweep_sequence(2024, a.base)[0]
    rows = min([a.rows] + [len(r) for r in raw])
    sweeps = torch.from_numpy(np.stack([np.asarray(r)[:rows, :3] for r in raw]).astype(np.float32)).to(dev)
    clouds = torch.from_numpy(synthetic.kitti_like_sequence(2024, a.npoints, a.base)[0]).to(dev)[:, :, :3].contiguous()
    period = 2 * (a.base - 1)
    order = [min(k % period, period - k % period) for k in range(a.frames + 40)]
    res = {"tool": "projective_bench", "rows": rows, "height": a.height, "width": a.width, "npoints": a.npoints,
           "map_size": a.map_size, "iters": a.iters, "frames": a.frames, "repeats": a.repeats,
           "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES")}
    for S in (1, 8):
        pick = [torch.tensor([order[k + i] for i in range(S)], device=dev) for k in range(a.frames)]
        proj = ProjectiveIcpRefiner(S, rows, height=a.height, width=a.width, map_size=a.map_size, iters=a.iters, graph=True)
        knn = IcpRefiner(S, a.npoints, map_size=a.map_size, iters=a.iters, graph=True)
        eye = torch.eye(4, dtype=torch.float64, device=dev).expand(S, 4, 4).contiguous()
        lengths = torch.full((S,), rows, dtype=torch.int32, device=dev)
        sweep_batches = [sweeps[p].contiguous() for p in pick]
        cloud_batches = [clouds[p].contiguous() for p in pick]

        def proj_pass():
            proj.reset()
            proj.register(sweep_batches[0], lengths, eye)
            return _per_frame_ms(lambda k: proj.register(sweep_batches[k], lengths, eye), a.frames)

        def knn_pass():
            knn.reset()
            knn.register(cloud_batches[0], eye)
            return _per_frame_ms(lambda k: knn.register(cloud_batches[k], eye), a.frames)

        proj_pass(), proj_pass(), knn_pass(), knn_pass()                        # warm-up and captures
        tp, tk = [], []
        for _ in range(a.repeats):
            tp.append(proj_pass())
            tk.append(knn_pass())
        dp, dk = proj.diagnostics(), knn.diagnostics()
        res["s%d" % S] = {"projective_register_ms": _stats(tp), "knn_register_ms": _stats(tk),
                          "projective_over_knn": _stats(tp)["median"] / _stats(tk)["median"],
                          "projective_launches": 2 + 1 + 2 + 2 * a.iters + 2, "knn_launches": 4 + 4 * a.iters + 1,
                          "projective_last_status": proj.status().tolist(), "projective_last_pairs": dp["pairs"].tolist(),
                          "projective_last_iterations": dp["iterations"].tolist(),
                          "knn_last_status": knn.status().tolist(), "knn_last_pairs": dk["pairs"].tolist()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
