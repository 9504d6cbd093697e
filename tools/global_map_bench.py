"""Times the global map on the device beside what a user would write in torch on the same device.

    python tools/global_map_bench.py [--repeats 9] [--out profiles/global_map/global_map_bench.jsonl]

Per stream count (1 and 8) at max_keyframes = 1024, n = 8192: one ``rebuild`` of a full bank (captured, replayed) and the
same map in torch (batched fp64 transform, voxel hash, ``torch.unique``, sort of the first indices), alternated in one
process, medians and spread over ``--repeats`` timed runs between two events on the stream; then one streaming ``advance``
(``max_new = 1``) onto a half-full bank.  Last, one ``StreamingOdometry`` step with and without ``map=``, alternated.  Prints
one JSON line per stream count and one for the step.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pwclonet_pylidarslam_amd import _lib                               # noqa: E402
from pwclonet_pylidarslam_amd.global_map import GlobalMap               # noqa: E402

K0, K1, K2 = 73856093, 19349669, 83492791


def path(S, frames, seed=3):
    """(frames, S, 4, 4) fp64: a sensor that moves about a metre a frame and turns slowly."""
    rng = np.random.default_rng(seed)
    X = np.zeros((frames, S, 4, 4))
    for s in range(S):
        yaw, pos = 0.0, np.zeros(3)
        for f in range(frames):
            c, sn = np.cos(yaw), np.sin(yaw)
            X[f, s] = [[c, -sn, 0.0, pos[0]], [sn, c, 0.0, pos[1]], [0.0, 0.0, 1.0, pos[2]], [0.0, 0.0, 0.0, 1.0]]
            yaw += rng.normal() * 0.02
            pos = pos + np.array([np.cos(yaw), np.sin(yaw), 0.0]) * rng.uniform(0.5, 1.5)
    return X


def fill(gm, X, seed=5):
    """A full bank straight into the buffers: every keyframe a sweep-like cloud around the sensor (the map does not care
    how the bank was filled)."""
    b, S, MK, n = gm.bufs, gm.streams, gm.max_keyframes, gm.num_points
    g = torch.Generator(device=gm.device).manual_seed(seed)
    for s in range(S):
        rad = torch.rand((MK, n), generator=g, device=gm.device) * 60.0 + 2.0
        ang = (torch.rand((MK, n), generator=g, device=gm.device) * 2.0 - 1.0) * np.pi
        z = torch.rand((MK, n), generator=g, device=gm.device) * 4.0 - 1.7
        b["bank_cloud"][s].copy_(torch.stack([rad * torch.cos(ang), rad * torch.sin(ang), z], dim=2))
    b["bank_frame"].copy_(torch.arange(MK, dtype=torch.int32, device=gm.device).expand(S, MK))
    b["bank_len"].fill_(n)
    b["state"][:, 0] = MK


def torch_map(bank, frames, X, v):
    """The same map in torch, stream by stream (``torch.unique`` is not batched): -> the winners' count per stream."""
    totals = []
    for s in range(bank.shape[0]):
        T = X[frames[s].long(), s]                                              # (MK, 4, 4)
        w = (bank[s].double() @ T[:, :3, :3].transpose(1, 2) + T[:, None, :3, 3]).float().reshape(-1, 3)
        q = torch.round(w.double() / v).long()
        h = q[:, 0] * K0 + q[:, 1] * K1 + q[:, 2] * K2
        uniq, inv = torch.unique(h, return_inverse=True)
        first = torch.full((uniq.shape[0],), h.shape[0], dtype=torch.int64, device=h.device)
        first.scatter_reduce_(0, inv, torch.arange(h.shape[0], device=h.device), "amin")
        win = first.sort().values
        points = w[win]
        totals.append(int(points.shape[0]))
    return totals


def event_time(fn, inner=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner * 1e3


def summary(t):
    return dict(median_us=statistics.median(t), min_us=min(t), max_us=max(t), repeats=len(t))


def captured(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with _lib.capture(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def maps(dev, repeats, points, keyframes, voxel):
    lines = []
    for S in (1, 8):
        gm = GlobalMap(S, points, voxel_size=voxel, max_keyframes=keyframes, graph=False, device=dev)
        gm._alloc()
        X = torch.from_numpy(path(S, keyframes)).to(dev)
        fill(gm, X)
        rebuild = captured(lambda: gm._body(1, X))
        ours = gm.totals().tolist()
        theirs = torch_map(gm.bufs["bank_cloud"], gm.bufs["bank_frame"], X, voxel)       # warm-up too
        t = dict(rebuild=[], torch=[])
        for _ in range(repeats):
            t["rebuild"].append(event_time(rebuild.replay))
            t["torch"].append(event_time(lambda: torch_map(gm.bufs["bank_cloud"], gm.bufs["bank_frame"], X, voxel)))
        half = keyframes // 2
        gm.bufs["cloud"].copy_(gm.bufs["bank_cloud"][:, 0])
        gm.bufs["lengths"].fill_(points)

        def halve():
            gm.bufs["state"][:, 0] = half
            gm.bufs["frame_id"].fill_(half)
        halve()
        gm._body(1, X)                                                       # the map of the first half
        advance = captured(lambda: gm._body(0, X))
        adv = []
        for _ in range(repeats):
            halve()
            gm._body(1, X)
            torch.cuda.synchronize()
            adv.append(event_time(advance.replay))                           # one keyframe onto a half-full map
        line = dict(streams=S, max_keyframes=keyframes, points=points, voxel_size=voxel, totals=ours, torch_totals=theirs,
                    rebuild=summary(t["rebuild"]), torch=summary(t["torch"]), advance=summary(adv), map_bytes=gm.map_bytes())
        print(json.dumps(line), flush=True)
        lines.append(line)
        del gm, rebuild, advance
        torch.cuda.empty_cache()
    return lines


def step_with_and_without(dev, repeats, points, voxel, frames=21):
    """One ``StreamingOdometry`` step with and without ``map=``, alternated in one process: per-frame medians of a pass over
    ``frames`` frames, ``repeats`` passes each, S = 1 and 8."""
    from pwclonet_pylidarslam_amd import synthetic
    from pwclonet_pylidarslam_amd.odometry import StreamingOdometry
    from pwclonet_pylidarslam_amd.pwclonet import PWCLONet
    base = torch.from_numpy(synthetic.kitti_like_sequence(2024, points, frames)[0]).to(dev)[:, :, :3].contiguous()
    torch.manual_seed(1234)
    net = PWCLONet(dict(num_input_channels=3, sequence_len=2, device=str(dev), scalar_last=False, log_mode="none"))
    net = net.to(dev).eval().prepare_fused()
    out = {}
    for S in (1, 8):
        batches = [base[torch.tensor([(k + 2 * i) % frames for i in range(S)], device=dev)] for k in range(frames)]
        sos = dict(plain=StreamingOdometry(net, streams=S, max_frames=frames + 1),
                   map=StreamingOdometry(net, streams=S, max_frames=frames + 1,
                                         map=dict(voxel_size=voxel, max_keyframes=1024)))

        def one_pass(so):
            so.reset()
            so.step(batches[0])
            t = []
            for k in range(1, frames):
                t.append(event_time(lambda: so.step(batches[k])))
            return statistics.median(t)
        for so in sos.values():
            one_pass(so), one_pass(so)                                       # eager call, capture
        times = dict(plain=[], map=[])
        for _ in range(repeats):
            for name, so in sos.items():
                times[name].append(one_pass(so))
        out["s%d" % S] = {name: summary(t) for name, t in times.items()}
        out["s%d" % S]["map_totals_last_pass"] = sos["map"].global_map().totals().tolist()
        del sos
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--keyframes", type=int, default=1024)
    ap.add_argument("--voxel", type=float, default=0.3)
    ap.add_argument("--no-step", action="store_true", help="leave out the StreamingOdometry step")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 7:
        raise SystemExit("--repeats must be >= 7")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    lines = maps(dev, args.repeats, args.points, args.keyframes, args.voxel)
    if not args.no_step:
        line = dict(step=step_with_and_without(dev, args.repeats, args.points, args.voxel))
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
