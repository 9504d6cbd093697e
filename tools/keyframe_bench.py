#!/usr/bin/env python3
"""What the keyframe gate of the knn refiner costs and what it does on a crawl; one JSON line.

(a) Cost.  ``IcpRefiner(graph=True)`` at n = 8192, map_size = 4, iters = 10, S = 1 and S = 8, on the frames and with the
timing of ``tools/icp_bench.py`` (HIP events around one ``register`` call, a sync after it, median over the frames of a
repeat): ``keyframe=None`` (the path without the gate), ``keyframe=dict(trans=0, rot=0)`` (the gate launched, every frame
inserted: the same maps, so the difference is the launch) and the reference's thresholds ``dict(trans=0.1, rot=0.3)``
(fewer inserts, so the maps differ too).  One process, the three alternated repeat by repeat; median / min / max over
``--repeats`` repeats.  The guess is the identity, as there.

(b) Crawl.  The box room of ``tests/icp_model.py`` walked 1 cm per frame along a fixed direction (``tests/keyframe_model.py:
room_walk``), ``--crawl-frames`` frames of n = 1024 points with 0.01 m range noise, map_size = 4, the guess "no motion":
the refined poses are chained and the last absolute pose is compared with the truth (metres + radians,
``icp_model.pose_error``), with ``keyframe=None`` and with the reference's thresholds, on the device and through the fp64
model on the same frames.  ``--model-only`` runs the model's half without a GPU, ``--no-model`` leaves it out.

    python tools/keyframe_bench.py [--frames F] [--repeats R] [--npoints N] [--crawl-frames K] [--no-model | --model-only]

The projective refiner has no keyframe gate, so neither half runs it.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import icp_model as model  # noqa: E402
import keyframe_model as kf  # noqa: E402
from pwclonet_pylidarslam_amd import synthetic  # noqa: E402
from pwclonet_pylidarslam_amd.registration import IcpRefiner  # noqa: E402

REFERENCE = dict(trans=0.1, rot=0.3)            # icp_odometry.py: threshold_trans, threshold_rot
EVERY = dict(trans=0.0, rot=0.0)


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


def cost(a, S, batches, dev):
    kw = dict(map_size=a.map_size, iters=a.iters, graph=True)
    refs = {"none": IcpRefiner(S, a.npoints, **kw), "every": IcpRefiner(S, a.npoints, keyframe=EVERY, **kw),
            "reference": IcpRefiner(S, a.npoints, keyframe=REFERENCE, **kw)}
    eye = torch.eye(4, dtype=torch.float64, device=dev).expand(S, 4, 4).contiguous()

    def one_pass(ref):
        ref.reset()
        ref.register(batches[0], eye)
        return _per_frame_ms(lambda k: ref.register(batches[k], eye), a.frames)

    for ref in refs.values():                                                   # warm-up and captures
        one_pass(ref), one_pass(ref)
    times = {k: [] for k in refs}
    for _ in range(a.repeats):
        for k, ref in refs.items():
            times[k].append(one_pass(ref))
    out = {"%s_register_ms" % k: _stats(v) for k, v in times.items()}
    med = {k: _stats(v)["median"] for k, v in times.items()}
    out.update(every_minus_none_us=1000.0 * (med["every"] - med["none"]),
               reference_minus_none_us=1000.0 * (med["reference"] - med["none"]),
               launches={"none": 4 + 4 * a.iters + 1, "keyframe": 4 + 4 * a.iters + 2},
               reference_inserted_of_frames=[refs["reference"].keyframe_state()["count"].tolist(), a.frames],
               last_pairs={k: r.diagnostics()["pairs"].tolist() for k, r in refs.items()})
    return out


def _final_error(rel, gt):
    acc, truth = np.eye(4), np.eye(4)
    for T, G in zip(rel, gt):
        acc, truth = acc @ T, truth @ G
    return model.pose_error(acc, truth)


def crawl_model(clouds, gt, M, iters, keyframe):
    mp, rel, inserts = model.Map(M, clouds.shape[1], 10), [], 0
    gate = None if keyframe is None else kf.Gate(**keyframe)
    for k in range(clouds.shape[0]):
        T, _, _ = model.register(mp, clouds[k], np.eye(4), iters=iters, push=False)
        ins = 1 if gate is None else gate.step(T, bool(mp.live.any()))
        kf.push(mp, clouds[k], T, ins)
        inserts += ins
        rel.append(T)
    return {"final_pose_error": _final_error(rel, gt), "inserted": inserts}


def crawl_device(clouds, gt, M, iters, keyframe, dev):
    ref = IcpRefiner(1, clouds.shape[1], map_size=M, iters=iters, graph=True, keyframe=keyframe)
    eye = torch.eye(4, dtype=torch.float64, device=dev)[None].contiguous()
    rel, inserts, froze = [], 0, 0
    for k in range(clouds.shape[0]):
        T = ref.register(torch.from_numpy(clouds[k][None]).to(dev), eye)
        rel.append(T[0].cpu().numpy().copy())
        inserts += 1 if keyframe is None else int(ref.keyframe_state()["insert"][0])
        froze += int(k > 0 and (int(ref.status()[0]) & (model.FEW_PAIRS | model.BAD_PIVOT)) != 0)
    return {"final_pose_error": _final_error(rel, gt), "inserted": inserts, "frames_without_a_solve": froze}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=41)
    ap.add_argument("--base", type=int, default=21, help="frames generated; the streams bounce through them")
    ap.add_argument("--npoints", type=int, default=8192)
    ap.add_argument("--map-size", type=int, default=4)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--crawl-frames", type=int, default=40)
    ap.add_argument("--crawl-points", type=int, default=1024)
    ap.add_argument("--crawl-step", type=float, default=0.01, help="metres per frame")
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--model-only", action="store_true")
    a = ap.parse_args()
    res = {"tool": "keyframe_bench", "npoints": a.npoints, "map_size": a.map_size, "iters": a.iters, "frames": a.frames,
           "repeats": a.repeats, "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES")}
    clouds, gt = kf.room_walk(3, kf.steps([a.crawl_step] * (a.crawl_frames - 1), deg=0.0), a.crawl_points)
    crawl = {"frames": a.crawl_frames, "step_m": a.crawl_step, "points": a.crawl_points, "noise_m": 0.01,
             "guess_final_pose_error": _final_error([np.eye(4)] * a.crawl_frames, gt)}
    if not a.model_only:
        dev = torch.device("cuda:0")
        torch.set_grad_enabled(False)
        base = torch.from_numpy(synthetic.kitti_like_sequence(2024, a.npoints, a.base)[0]).to(dev)[:, :, :3].contiguous()
        period = 2 * (a.base - 1)
        order = [min(k % period, period - k % period) for k in range(a.frames + 40)]
        for S in (1, 8):
            batches = [base[torch.tensor([order[k + 5 * i] for i in range(S)], device=dev)] for k in range(a.frames)]
            res["s%d" % S] = cost(a, S, batches, dev)
        crawl["device_none"] = crawl_device(clouds, gt, a.map_size, a.iters, None, dev)
        crawl["device_reference"] = crawl_device(clouds, gt, a.map_size, a.iters, REFERENCE, dev)
    if not a.no_model:
        crawl["model_none"] = crawl_model(clouds, gt, a.map_size, a.iters, None)
        crawl["model_reference"] = crawl_model(clouds, gt, a.map_size, a.iters, REFERENCE)
    res["crawl"] = crawl
    print(json.dumps(res))


if __name__ == "__main__":
    main()
