"""Times one loop detection on the device and the same exhaustive search restated in NumPy.

    python tools/loop_closure_bench.py [--repeats 9] [--out profiles/loop_closure/loop_closure_bench.jsonl]

Per (streams, stored places) at n = 8192: one captured replay of descriptor + score + select, and of the whole chain with
verification (fetch, two registrations, accept, insert), medians and spread over ``--repeats`` timed batches of replays
between two events on the stream; beside it the same search in NumPy on 16 host threads.  Then one ``StreamingOdometry``
step with and without ``loop=``, alternated in one process.  Prints one JSON line per size and one for the step.

    python tools/loop_closure_bench.py --translation [--out profiles/loop_closure/translation_bench.jsonl]

times instead the whole chain with and without ``translation=`` (its defaults), alternated in one process, for S = 1 and 8:
the yardstick of the translation search is the same chain without it at the same commit.
"""
import argparse
import concurrent.futures
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pwclonet_pylidarslam_amd import _lib                              # noqa: E402
from pwclonet_pylidarslam_amd.loop_closure import ScanContextLoopDetector   # noqa: E402


def cloud(seed, S, n):
    rng = np.random.default_rng(seed)
    rad, ang = rng.uniform(1.0, 70.0, (S, n)), rng.uniform(-np.pi, np.pi, (S, n))
    return np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-1.5, 3.0, (S, n))], axis=2).astype(np.float32)


def fill(det, places, seed):
    """Random normalised places straight into the database (the search does not care how they got there)."""
    b, rng = det.bufs, np.random.default_rng(seed)
    S, NR, NS = det.streams, det.rings, det.sectors
    D = rng.uniform(0.1, 4.0, (S, places, NS, NR)).astype(np.float32)
    D /= np.sqrt((D * D).sum(axis=3, keepdims=True))
    b["db_desc"][:, :places].copy_(torch.from_numpy(D))
    b["db_mask"][:, :places].fill_((1 << NS) - 1)
    b["db_frame"][:, :places].copy_(torch.arange(places, dtype=torch.int32).expand(S, places))
    b["count"].fill_(places)
    b["db_cloud"][:, :places].copy_(torch.from_numpy(cloud(seed + 1, S, det.num_points)).to(b["db_cloud"].device)[:, None])
    # place 0 is the query itself, so that every replay finds, fetches, registers and accepts
    b["db_desc"][:, 0].copy_(b["Dn"].transpose(1, 2))
    b["db_mask"][:, 0].copy_(b["qmask"])
    b["db_cloud"][:, 0].copy_(b["cloud"])
    return D


def timed(fn, repeats, inner=10):
    g = torch.cuda.CUDAGraph()
    fn()
    torch.cuda.synchronize()
    with _lib.capture(g):
        fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            g.replay()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / inner * 1e3)
    return dict(median_us=statistics.median(out), min_us=min(out), max_us=max(out))


THREADS = 16


def numpy_search(Qn, D, pool):
    """min over shifts of 1 - (column-wise correlation) / NS, every place, full masks: one matrix-vector product per shift,
    the shifts spread over ``THREADS`` host threads (NumPy releases the interpreter lock inside the product)."""
    NR, NS = Qn.shape
    E = D.reshape(len(D), NS * NR)                                       # (places, NS, NR) flattened: a column is contiguous
    one = lambda s: 1.0 - (E @ np.ascontiguousarray(np.roll(Qn, -s, axis=1).T).reshape(-1)) / NS
    best = np.minimum.reduce(list(pool.map(one, range(NS))))
    return int(best.argmin())


def step_with_and_without(dev, repeats, points, frames=21):
    """One ``StreamingOdometry`` step with and without ``loop=``, alternated in one process: per-frame medians of a pass over
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
        sos = dict(plain=StreamingOdometry(net, streams=S, max_frames=frames + 1, backend=dict(source="network")),
                   loop=StreamingOdometry(net, streams=S, max_frames=frames + 1, backend=dict(source="network"),
                                          loop=dict(min_id_distance=5, max_keyframes=1024)))

        def one_pass(so):
            so.reset()
            so.step(batches[0])
            t = []
            for k in range(1, frames):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                so.step(batches[k])
                b.record()
                b.synchronize()
                t.append(a.elapsed_time(b) * 1e3)
            return statistics.median(t)
        for so in sos.values():
            one_pass(so), one_pass(so)                                   # eager call, capture
        times = dict(plain=[], loop=[])
        for _ in range(repeats):
            for name, so in sos.items():
                times[name].append(one_pass(so))
        out["s%d" % S] = {name: dict(median_us=statistics.median(t), min_us=min(t), max_us=max(t)) for name, t in times.items()}
        out["s%d" % S]["accepted_last_pass"] = len(sos["loop"].loop_detector().loops())
    return out


def replays(graph, inner=10):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner * 1e3


def chain_with_and_without(dev, repeats, points, places=1024):
    """The whole chain (every replay finds, fetches, registers and accepts place 0, the query itself) with and without
    ``translation=``, one captured graph each, timed in alternation: -> one line per stream count."""
    lines = []
    for S in (1, 8):
        frames = torch.from_numpy(cloud(7, S, points)).to(dev)
        dets, graphs = {}, {}
        for name, tr in (("plain", None), ("translation", dict())):
            det = ScanContextLoopDetector(S, points, max_keyframes=places + 8, min_id_distance=0, device=dev, translation=tr)
            det.process(frames, [places] * S)
            fill(det, places, 11)

            def chain(det=det):
                det.bufs["count"].fill_(places)
                det._body(None)
            chain()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with _lib.capture(g):
                chain()
            for _ in range(3):
                g.replay()
            torch.cuda.synchronize()
            dets[name], graphs[name] = det, g
        times = dict(plain=[], translation=[])
        for _ in range(repeats):
            for name in times:
                times[name].append(replays(graphs[name]))
        seed = dets["translation"].seed()
        line = dict(streams=S, places=places, points=points, parameters=dets["translation"].translation,
                    seed_found=seed["found"].tolist(), seed_cells=seed["occ_q"].tolist(),
                    accepted=dets["translation"].match()["accepted"].tolist())
        line.update({name: dict(median_us=statistics.median(t), min_us=min(t), max_us=max(t)) for name, t in times.items()})
        print(json.dumps(line), flush=True)
        lines.append(line)
        del dets, graphs
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--out", default=None)
    ap.add_argument("--translation", action="store_true", help="the whole chain with and without translation=, alternated")
    args = ap.parse_args()
    if args.repeats < 7:
        raise SystemExit("--repeats must be >= 7")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    if args.translation:
        lines = chain_with_and_without(dev, args.repeats, args.points)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                for line in lines:
                    f.write(json.dumps(line) + "\n")
        return
    pool = concurrent.futures.ThreadPoolExecutor(THREADS)
    lines = []
    for S in (1, 8):
        for places in (1024, 4096):
            det = ScanContextLoopDetector(S, args.points, max_keyframes=places + 8, min_id_distance=0, device=dev)
            frames = torch.from_numpy(cloud(7, S, args.points)).to(dev)
            det.process(frames, [places] * S)                            # allocates, primes the refiner
            D = fill(det, places, 11)
            search = timed(det.search, args.repeats)

            def chain():
                det.bufs["count"].fill_(places)                          # every replay searches the same database
                det._body(None)
            whole = timed(chain, args.repeats)
            Qn = det.bufs["Dn"][0].cpu().numpy()
            t = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                numpy_search(Qn, D[0], pool)
                t.append((time.perf_counter() - t0) * 1e6)
            line = dict(streams=S, places=places, points=args.points, search=search, chain=whole,
                        numpy_one_stream=dict(median_us=statistics.median(t), min_us=min(t), max_us=max(t)),
                        found=det.match()["found"].tolist(), map_bytes=det.map_bytes())
            print(json.dumps(line), flush=True)
            lines.append(line)
            del det
            torch.cuda.empty_cache()
    line = dict(step=step_with_and_without(dev, args.repeats, args.points))
    print(json.dumps(line), flush=True)
    lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
