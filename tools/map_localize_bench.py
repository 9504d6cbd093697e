"""Times localisation in the global map beside the two refiners that register against local maps.

    python tools/map_localize_bench.py [--repeats 9] [--keyframes 1024] [--out profiles/map_localize/map_localize_bench.jsonl]

Per stream count (1 and 8) at max_keyframes = 1024, n = 8192, v = 0.3 and a full bank: one ``localize`` replay at radius 1
and 2, alternated in one process with ``VoxelMapRefiner.register`` and ``IcpRefiner.register`` at the same n and iters; the
accumulate kernel alone at both radii beside ``voxel_accumulate_kernel`` alone (section 24's yardstick, same run); the full
index pass and one append pass after a single ``advance``.  Medians and spread = (max - min) / median over ``--repeats``
timed runs between two events on the stream.  One JSON line per stream count, and one for a ``StreamingOdometry`` step
with ``map=`` alone and with ``map=`` and ``localize=``, alternated (``--no-step`` leaves it out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import global_map_bench as gmb                                             # noqa: E402  (path, fill, event_time)
from pwclonet_pylidarslam_amd import _lib, map_localize, voxel_map        # noqa: E402
from pwclonet_pylidarslam_amd.global_map import GlobalMap                  # noqa: E402
from pwclonet_pylidarslam_amd.map_localize import MapLocalizer             # noqa: E402
from pwclonet_pylidarslam_amd.registration import IcpRefiner               # noqa: E402
from pwclonet_pylidarslam_amd.voxel_map import VoxelMapRefiner             # noqa: E402


def stats(times):
    med = statistics.median(times)
    return dict(median_us=round(med, 1), spread=round((max(times) - min(times)) / med, 3))


def alternate(fns, repeats, warm=3):
    """name -> callable, timed in turn so that all see the same clocks."""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            out[k].append(gmb.event_time(fn))
    return {k: stats(v) for k, v in out.items()}


def run(S, MK, n, v, iters, repeats, dev):
    X = torch.from_numpy(gmb.path(S, MK)).to(dev)
    gm = GlobalMap(S, n, v, max_keyframes=MK, device=dev)
    gm._alloc()
    gmb.fill(gm, X)
    gm.rebuild(X)
    gm.rebuild(X)
    b = gm.bufs
    mid = MK // 2
    cloud = b["bank_cloud"][:, mid].contiguous()                           # a banked frame, localised from a guess 0.2 m off
    guess = X[mid].clone()
    guess[:, :3, 3] += 0.2
    res = dict(S=S, max_keyframes=MK, n=n, voxel_size=v, iters=iters, totals=gm.totals().tolist())
    locs = {R: MapLocalizer(gm, radius=R, iters=iters) for R in (1, 2)}
    for loc in locs.values():
        loc.index()
    vox = VoxelMapRefiner(S, n, iters=iters)
    knn = IcpRefiner(S, n, iters=iters)
    eye = torch.eye(4, dtype=torch.float64, device=dev).expand(S, 4, 4).contiguous()
    fns = {"localize_r1": lambda: locs[1].localize(cloud, guess), "localize_r2": lambda: locs[2].localize(cloud, guess),
           "voxel_map_register": lambda: vox.register(cloud, eye), "icp_register": lambda: knn.register(cloud, eye)}
    res.update(alternate(fns, repeats))
    res["localize_pairs"] = {R: locs[R].diagnostics()["pairs"].tolist() for R in (1, 2)}
    # the accumulate kernels alone, section 24's beside this section's
    args = (b["keys"], b["rows"], b["points"], b["source"], gm.totals(), locs[1].bufs["index"], v, cloud, guess)
    vb = vox.bufs
    fns = {"map_accumulate_r1": lambda: map_localize.accumulate(*args, radius=1),
           "map_accumulate_r2": lambda: map_localize.accumulate(*args, radius=2),
           "voxel_accumulate": lambda: voxel_map.accumulate(vb["grid"], vox.extent, vox.voxel_size, cloud, vb["P"], vb["T"])}
    res.update(alternate(fns, repeats))
    # the index: in full, and what one advance appended
    loc = locs[1]
    res["index_full"] = stats([gmb.event_time(lambda: loc.index()) for _ in range(repeats + 2)][2:])
    gm2 = GlobalMap(S, n, v, max_keyframes=MK, device=dev)
    gm2._alloc()
    gmb.fill(gm2, X)
    gm2.bufs["state"][:, 0] = mid
    gm2.rebuild(X)
    loc2 = MapLocalizer(gm2)
    loc2.index()
    ids = torch.full((S,), mid, dtype=torch.int32, device=dev)
    times = []
    for k in range(repeats + 2):
        ids.fill_(mid + k)
        gm2.advance(b["bank_cloud"][:, mid + k].contiguous(), ids, X)
        times.append(gmb.event_time(lambda: loc2.index(full=False)))
    res["index_append"] = stats(times[2:])
    res["index_bytes"] = loc.index_bytes()
    _lib.synchronize(dev)
    return res


def step_with_and_without(dev, repeats, points, voxel, frames=21):
    """One ``StreamingOdometry`` step with ``map=`` alone and with ``localize=`` on top, alternated in one process:
    per-frame medians of a pass over ``frames`` frames, ``repeats`` passes each, S = 1 and 8 (global_map_bench's scheme).
    ``min_id_distance=5``, so that from the sixth frame of a pass on the gate lets old frames attract."""
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
        kw = dict(streams=S, max_frames=frames + 1, map=dict(voxel_size=voxel, max_keyframes=1024))
        sos = dict(map=StreamingOdometry(net, **kw),
                   localize=StreamingOdometry(net, localize=dict(min_id_distance=5), **kw))

        def one_pass(so):
            so.reset()
            so.step(batches[0])
            t = []
            for k in range(1, frames):
                t.append(gmb.event_time(lambda: so.step(batches[k])))
            return statistics.median(t)
        for so in sos.values():
            one_pass(so), one_pass(so)                                       # eager call, capture
        times = dict(map=[], localize=[])
        for _ in range(repeats):
            for name, so in sos.items():
                times[name].append(one_pass(so))
        out["s%d" % S] = {name: stats(t) for name, t in times.items()}
        out["s%d" % S]["pairs_last_step"] = sos["localize"].localizer().diagnostics()["pairs"].tolist()
        del sos
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--keyframes", type=int, default=1024)
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--streams", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--no-step", action="store_true", help="leave out the StreamingOdometry step")
    ap.add_argument("--out", default=os.path.join("profiles", "map_localize", "map_localize_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    lines = [run(S, a.keyframes, a.points, 0.3, a.iters, a.repeats, dev) for S in a.streams]
    if not a.no_step:
        lines.append(dict(step=step_with_and_without(dev, a.repeats, a.points, 0.3)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
