#!/usr/bin/env python3
"""Bringing the packed eval-mode weights up to date: a full re-pack (``prepare_fused()``, the only way before
``refresh_fused()`` existed) against the in-place refresh, one process, alternated and repeated; prints one JSON line.

Per repeat, on the same network (weights edited in place before each measurement, as an optimizer step would):
(a) ``prepare_fused()`` and ``refresh_fused()``: host wall time of the call (returns with work still queued) and the
    device time between HIP events recorded around it (for the re-pack that span includes the idle gaps between its
    many small launches: it is the time the stream is busy with the update, not a sum of kernel times);
(b) the first ``StreamingOdometry.step`` (S = 1, graph=True) after each, host clock around the call plus a device
    synchronise: after a re-pack the odometry meets a new ``_fused`` object, drops its graphs, warms up and captures
    again; after a refresh it replays.  The steady step (no update before it) is timed the same way for scale.
Checks: after every refresh the packed buffers equal a fresh pack bit for bit; the odometry's graph objects change
after a re-pack and stay after a refresh.

    python tools/refresh_bench.py [--repeats R] [--npoints N] [--dtype f32|bf16x3|bf16]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pwclonet_pylidarslam_amd import fused, synthetic  # noqa: E402
from pwclonet_pylidarslam_amd.odometry import StreamingOdometry  # noqa: E402
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet  # noqa: E402


def _stats(xs):
    xs = sorted(xs)
    med = xs[len(xs) // 2]
    return {"median": med, "min": xs[0], "max": xs[-1], "spread_pct": 100.0 * (xs[-1] - xs[0]) / med}


def _timed_call(dev, fn):
    """(host ms until fn returns, device ms between events around it, host ms until the device is idle)."""
    torch.cuda.synchronize(dev)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    s.record()
    fn()
    e.record()
    t1 = time.perf_counter()
    e.synchronize()
    t2 = time.perf_counter()
    return 1e3 * (t1 - t0), s.elapsed_time(e), 1e3 * (t2 - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--npoints", type=int, default=8192)
    ap.add_argument("--dtype", default="f32")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    torch.manual_seed(1234)
    net = PWCLONet(dict(num_input_channels=3, sequence_len=2, device=str(dev), scalar_last=False,
                        log_mode="none")).to(dev).eval()
    net.prepare_fused(dtype=a.dtype)
    base = torch.from_numpy(synthetic.kitti_like_sequence(2024, a.npoints, 8)[0]).to(dev)[:, :, :3].contiguous()
    frame = lambda k: base[k % base.shape[0]][None]
    so = StreamingOdometry(net, streams=1, max_frames=4096, graph=True)
    k = 0
    for _ in range(4):                                   # prime + steps: the graph exists, everything is warm
        so.step(frame(k))
        k += 1
    net.refresh_fused()                                  # warm: the refresh kernel's code object
    torch.cuda.synchronize(dev)

    def edit():
        for p in net.parameters():
            p.mul_(1.0009765625)                         # an in-place edit of every parameter (version counters move)

    def graph():
        entry = next(iter(so._graphs.values()), None)
        return None if entry is None else entry["step"] and entry["step"][0]

    rows = {n: [] for n in ("prepare_host_ms", "prepare_device_ms", "prepare_until_idle_ms", "refresh_host_ms",
                            "refresh_device_ms", "refresh_until_idle_ms", "step_after_prepare_ms", "step_after_refresh_ms",
                            "step_steady_ms")}
    recaptured, kept, equal = [], [], []
    for _ in range(a.repeats):
        # the parent path: pack again, then the odometry captures again
        edit()
        old, g0 = net._fused, graph()                    # (kept alive: a new object must not reuse the old one's id)
        h, d, w = _timed_call(dev, lambda: net.prepare_fused())
        rows["prepare_host_ms"].append(h), rows["prepare_device_ms"].append(d), rows["prepare_until_idle_ms"].append(w)
        rows["step_after_prepare_ms"].append(_timed_call(dev, lambda: so.step(frame(k)))[2])
        k += 1
        recaptured.append(net._fused is not old and graph() is not g0)
        del old
        rows["step_steady_ms"].append(_timed_call(dev, lambda: so.step(frame(k)))[2])
        k += 1
        # the new path: refresh in place, the odometry replays
        edit()
        obj, g0 = net._fused, graph()
        h, d, w = _timed_call(dev, lambda: net.refresh_fused())
        rows["refresh_host_ms"].append(h), rows["refresh_device_ms"].append(d), rows["refresh_until_idle_ms"].append(w)
        rows["step_after_refresh_ms"].append(_timed_call(dev, lambda: so.step(frame(k)))[2])
        k += 1
        kept.append(net._fused is obj and graph() is g0)
        with fused.packing_dtype(a.dtype):
            fresh = fused.FusedPWCLONet(net).packed_buffers()
        equal.append(all(torch.equal(t.view(torch.int32), fresh[n].view(torch.int32))
                         for n, t in net._fused.packed_buffers().items()))
    plan = net._fused.plan
    res = {"tool": "refresh_bench", "npoints": a.npoints, "dtype": a.dtype, "repeats": a.repeats, "streams": 1,
           "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "plan_jobs": len(plan.jobs), "plan_tiles": plan.total_tiles,
           "packed_bytes": 4 * sum(j.floats for j in plan.jobs)}
    res.update({n: _stats(v) for n, v in rows.items()})
    res["graphs_recaptured_after_prepare"] = all(recaptured)
    res["graphs_kept_after_refresh"] = all(kept)
    res["refreshed_buffers_bitwise_equal_fresh_pack"] = all(equal)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
