#!/usr/bin/env python3
"""The voxel-map refiner beside the knn refiner, one process; one JSON line.

Table 1: the HIP-event time of one ``register`` replay (one frame in flight: events around the call, a sync after it;
median over the frames of a pass) of ``VoxelMapRefiner`` (default map) and of ``IcpRefiner(map_size=4)`` at n = 8192,
iters = 10, S = 1 and S = 8, alternated pass by pass, median (min-max) over ``--repeats`` passes; launches per replay and
map bytes.  The guess is the identity, as in ``tools/icp_bench.py``.

Table 2: a ``synthetic.kitti_like_sequence`` of ``--walk`` frames through ``StreamingOdometry`` with a network whose pose
heads say "no motion" (the suite's synthetic weights do not estimate a vehicle's motion): the distance between the final
position and the ground truth's for the network's trajectory, for ``refine=dict(kind="knn")`` and for
``refine=dict(kind="voxel_map")``, and the frames held in the voxel map at the end.

    python tools/voxel_map_bench.py [--frames F] [--repeats R] [--npoints N] [--iters I] [--walk W]
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
from pwclonet_pylidarslam_amd.odometry import StreamingOdometry  # noqa: E402
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet  # noqa: E402
from pwclonet_pylidarslam_amd.registration import IcpRefiner  # noqa: E402
from pwclonet_pylidarslam_amd.voxel_map import VoxelMapRefiner  # noqa: E402


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


def _timing(a, S, batches, dev):
    knn = IcpRefiner(S, a.npoints, map_size=4, iters=a.iters, graph=True)
    vox = VoxelMapRefiner(S, a.npoints, iters=a.iters, graph=True)
    eye = torch.eye(4, dtype=torch.float64, device=dev).expand(S, 4, 4).contiguous()

    def one_pass(ref):
        ref.reset()
        ref.register(batches[0], eye)
        return _per_frame_ms(lambda k: ref.register(batches[k], eye), a.frames)

    for ref in (knn, vox, knn, vox):                      # warm-up; the second pass of each replays only
        one_pass(ref)
    tk, tv = [], []
    for _ in range(a.repeats):
        tk.append(one_pass(knn))
        tv.append(one_pass(vox))
    return {"knn_register_ms": _stats(tk), "voxel_map_register_ms": _stats(tv),
            "voxel_map_over_knn": _stats(tv)["median"] / _stats(tk)["median"],
            "knn_launches_per_replay": 4 + 4 * a.iters + 1, "voxel_map_launches_per_replay": 1 + 3 + 2 * a.iters + 4,
            "voxel_map_bytes": vox.map_bytes(),
            "knn_map_bytes": sum(knn.bufs[k].numel() * knn.bufs[k].element_size() for k in ("map_xyz", "map_normals", "map_ws")),
            "voxel_map_last_pairs": vox.diagnostics()["pairs"].tolist(), "knn_last_pairs": knn.diagnostics()["pairs"].tolist()}


def _still_net(dev):
    torch.manual_seed(1234)
    net = PWCLONet(dict(num_input_channels=3, sequence_len=2, device=str(dev), scalar_last=False, log_mode="none"))
    sd = net.state_dict()
    for key, v in sd.items():
        if key.endswith(("conv1d_q.conv.weight", "conv1d_t.conv.weight", "conv1d_t.conv.bias")):
            v.zero_()
        elif key.endswith("conv1d_q.conv.bias"):
            v.copy_(torch.tensor([1.0, 0.0, 0.0, 0.0]))
    return net.to(dev).eval().prepare_fused()


def _walk(a, dev):
    pcs, q, t = synthetic.kitti_like_sequence(77, a.npoints, a.walk)
    truth = np.eye(4)
    for k in range(a.walk - 1):
        w, x, y, z = q[k].astype(np.float64)
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        step = np.eye(4)
        step[:3, :3], step[:3, 3] = R, t[k]
        truth = truth @ step
    frames = torch.from_numpy(pcs).to(dev)
    net = _still_net(dev)
    common = dict(iters=a.iters, max_dist=2.0)
    out = {"frames": a.walk, "truth_path_m": float(np.linalg.norm(t.astype(np.float64), axis=1).sum())}
    for name, refine in (("knn", dict(common, kind="knn", map_size=4)),
                         ("voxel_map", dict(common, kind="voxel_map", voxel_size=2.0, extent=(128, 32, 128)))):
        so = StreamingOdometry(net, streams=1, max_frames=a.walk + 1, graph=True, refine=refine)
        for k in range(a.walk):
            so.step(frames[k:k + 1])
        end = so.refined_trajectory()[-1, 0].cpu().numpy()
        out[name + "_final_error_m"] = float(np.linalg.norm(end[:3, 3] - truth[:3, 3]))
        if name == "knn":
            net_end = so.trajectory()[-1, 0].cpu().numpy()
            out["network_final_error_m"] = float(np.linalg.norm(net_end[:3, 3] - truth[:3, 3]))
        else:
            keys = so.refiner().map_points(0)["keys"]
            out["voxel_map_frames_held"] = int(torch.unique(keys >> 32).numel())
            out["voxel_map_points_held"] = int(keys.numel())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=41)
    ap.add_argument("--base", type=int, default=21, help="frames generated; the streams bounce through them")
    ap.add_argument("--npoints", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--walk", type=int, default=31, help="frames of the trajectory table")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    base = torch.from_numpy(synthetic.kitti_like_sequence(2024, a.npoints, a.base)[0]).to(dev)[:, :, :3].contiguous()
    period = 2 * (a.base - 1)
    order = [min(k % period, period - k % period) for k in range(a.frames + 40)]
    res = {"tool": "voxel_map_bench", "npoints": a.npoints, "iters": a.iters, "frames": a.frames, "repeats": a.repeats,
           "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES")}
    for S in (1, 8):
        batches = [base[torch.tensor([order[k + 5 * i] for i in range(S)], device=dev)] for k in range(a.frames)]
        res["s%d" % S] = _timing(a, S, batches, dev)
    res["walk"] = _walk(a, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
