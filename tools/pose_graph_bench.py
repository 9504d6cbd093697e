"""Measures one ``PoseGraph.optimize`` replay at KITTI 00's length and writes profiles/pose_graph/README.md and
pose_graph_bench.json.  Nothing is asserted.

    python tools/pose_graph_bench.py [--poses 4541] [--loops 20] [--streams 1 8] [--repeats 7] [--iters 20]
                                     [--pcg-iters N] [--skip-host] [--robust]

The problem: a noisy chain of ``--poses`` vertices per stream with ``--loops`` exact long-range measurements spread over it
(tests/pose_graph_cases.noisy_chain).  Per stream count, alternated over ``--repeats`` rounds, the graph is put back to its
odometry and one captured ``optimize`` of ``--iters`` LM iterations is replayed and timed with events: median (min - max).
Beside it: CG iterations used and the final relative residual per LM step, whether CG hit ``pcg_iters``, and the same problem
through the model's ``scipy.sparse.linalg.spsolve`` path on the host (the only baseline there is: g2o is not installed, so no
time against the reference exists).  ``--pcg-iters`` bounds one solve; the default is the constructor's 12 max_poses.

``--robust`` measures instead what a robust kernel costs: per stream count two graphs of the same
problem, one without a kernel and one with Geman-McClure, delta = 1, on the loops, replayed in turn in one process; the
yardstick is the plain replay of the same run.  It writes profiles/pose_graph_robust/ and skips the host baseline.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pose_graph_cases as pgc          # noqa: E402
import pose_graph_model as pgm          # noqa: E402


def problem(n, loops, seed):
    g, gt = pgc.noisy_chain(n, seed, ML=max(loops, 1), MA=1)
    rng = np.random.default_rng(seed + 1)
    for _ in range(loops):
        i = int(rng.integers(0, n // 2))
        j = int(rng.integers(n // 2, n))
        g.add_loop(i, j, pgc.between(gt, i, j))
    return g


def host_baseline(g, iters):
    """The model's LM with the sparse direct solve, assembled sparsely (the dense H of the tests does not fit at this size)."""
    import scipy.sparse
    import scipy.sparse.linalg
    t0 = time.perf_counter()
    lam = nu = None
    steps = 0
    for it in range(iters):
        slots, (ids, vi, vj, ab) = pgm.linearise(g, g.X)
        chi = pgm.block_sum(slots[:, pgm.CHI])
        rows, cols, vals = [], [], []
        for k, id_ in enumerate(ids):
            i, j = vi[k], vj[k]
            blocks = [(j, j, slots[id_, pgm.HJJ:pgm.HJJ + 36].reshape(6, 6))]
            if not ab[k]:
                hij = slots[id_, pgm.HIJ:pgm.HIJ + 36].reshape(6, 6)
                blocks += [(i, i, slots[id_, pgm.HII:pgm.HII + 36].reshape(6, 6)), (i, j, hij), (j, i, hij.T)]
            for r, c, m in blocks:
                rr, cc = np.meshgrid(np.arange(6) + 6 * r, np.arange(6) + 6 * c, indexing="ij")
                rows.append(rr.ravel()); cols.append(cc.ravel()); vals.append(m.ravel())
        n6 = 6 * g.n
        H = scipy.sparse.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n6, n6))
        b = pgm.gather_b(g, slots)
        idx = pgm.free_index(g)
        if it == 0:
            lam, nu = 1e-5 * H.diagonal()[idx].max(), 2.0
        if np.max(np.abs(b)) <= 1e-12:
            break
        A = (H + lam * scipy.sparse.identity(n6, format="csc"))[idx][:, idx]
        d = np.zeros(n6)
        d[idx] = scipy.sparse.linalg.spsolve(A.tocsc(), -b.reshape(-1)[idx])
        out = pgm.judge(g, g.X, d.reshape(-1, 6), b, lam, nu, chi)
        g.X, lam, nu = out["X"], out["lam"], out["nu"]
        steps += 1
        if out["status"]:
            break
    return dict(seconds=time.perf_counter() - t0, lm_steps=steps, chi2=float(out["chi"]), threads=os.cpu_count())


ROBUST = dict(kernel="geman_mcclure", delta=1.0, edges=("loop",))


def device_run(graphs, args, robust=None):
    from pwclonet_pylidarslam_amd.pose_graph import PoseGraph
    import pose_graph_device as pgd
    g0 = graphs[0]
    pg = PoseGraph(len(graphs), max_poses=g0.N, max_loops=g0.ML, max_absolute=g0.MA, iters=args.iters,
                   pcg_iters=args.pcg_iters, robust=robust)
    pgd.load(pg, graphs)
    start = {k: pg.bufs[k].clone() for k in ("X", "lam", "nu", "chi2", "status")}

    def once():
        for k, v in start.items():
            pg.bufs[k].copy_(v)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); pg.optimize(); b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)
    once(); once()                                       # eager, then the capture
    return pg, once


def robust_main(args):
    """Plain and robust replays of the same problems, alternated; the ratio is taken of the medians of one process."""
    out = args.out or os.path.join(ROOT, "profiles", "pose_graph_robust")
    runs = {}
    for S in args.streams:
        for name, robust in (("plain", None), ("robust", ROBUST)):
            runs[S, name] = device_run([problem(args.poses, args.loops, 100 + s) for s in range(S)], args, robust)
    times = {k: [] for k in runs}
    for _ in range(args.repeats):
        for k in runs:
            times[k].append(runs[k][1]())
    result = dict(poses=args.poses, loops=args.loops, iters=args.iters, repeats=args.repeats, robust=ROBUST, device={})
    lines = ["# Pose-graph backend: one `optimize` replay with and without a robust kernel", "",
             "`python tools/pose_graph_bench.py --robust` on one MI355X; the data is `pose_graph_robust_bench.json`.  N = %d poses, "
             "%d exact loops, %d LM iterations, %d repeats alternated between the two graphs in one process, median (min - "
             "max).  The kernel: Geman-McClure, delta = 1, on the loops.  The two graphs need not take the same LM path, so the "
             "CG iterations of each are listed; the kernel itself adds a few flops per edge to two of the four launches of an "
             "iteration." % (args.poses, args.loops, args.iters, args.repeats), "",
             "| streams | no kernel | with the kernel | ratio of medians | CG iterations, no kernel / kernel (stream 0, summed) |",
             "|---|---|---|---|---|"]
    for S in args.streams:
        row = {}
        for name in ("plain", "robust"):
            pg, t = runs[S, name][0], times[S, name]
            row[name] = dict(ms_median=float(np.median(t)), ms_min=float(np.min(t)), ms_max=float(np.max(t)), ms_all=t,
                             pcg_used=pg.bufs["pcg_used"].cpu().numpy().tolist(), status=pg.status().tolist(),
                             chi2=pg.chi2().tolist())
        row["min_loop_weight"] = float(torch.stack([runs[S, "robust"][0].loop_weights(s)[:, 1].min() for s in range(S)]).min())
        result["device"][str(S)] = row
        a, b = row["plain"], row["robust"]
        lines.append("| %d | %.1f ms (%.1f - %.1f) | %.1f ms (%.1f - %.1f) | %.3f | %d / %d |" % (
            S, a["ms_median"], a["ms_min"], a["ms_max"], b["ms_median"], b["ms_min"], b["ms_max"],
            b["ms_median"] / a["ms_median"], sum(a["pcg_used"][0]), sum(b["pcg_used"][0])))
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "pose_graph_robust_bench.json"), "w") as f:
        json.dump(result, f, indent=1)
    with open(os.path.join(out, "README.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps({"device_ms": {str(S): [result["device"][str(S)][n]["ms_median"] for n in ("plain", "robust")]
                                    for S in args.streams}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=4541)
    ap.add_argument("--loops", type=int, default=20)
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--pcg-iters", type=int, default=None)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--robust", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.robust:
        return robust_main(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "pose_graph")
    runs = {}
    for S in args.streams:
        runs[S] = device_run([problem(args.poses, args.loops, 100 + s) for s in range(S)], args)
    times = {S: [] for S in args.streams}
    for _ in range(args.repeats):                        # alternated
        for S in args.streams:
            times[S].append(runs[S][1]())
    result = dict(poses=args.poses, loops=args.loops, iters=args.iters, repeats=args.repeats, device={})
    for S in args.streams:
        pg = runs[S][0]
        used, rel = pg.bufs["pcg_used"].cpu().numpy(), pg.bufs["relres"].cpu().numpy()
        result["device"][str(S)] = dict(
            ms_median=float(np.median(times[S])), ms_min=float(np.min(times[S])), ms_max=float(np.max(times[S])),
            ms_all=times[S], pcg_iters=pg.pcg_iters, pcg_used=used.tolist(), relres=rel.tolist(),
            hit_pcg_iters=bool((used >= pg.pcg_iters).any()), status=pg.status().tolist(), chi2=pg.chi2().tolist(),
            accepted=pg.bufs["accepted"].cpu().numpy().tolist())
    if not args.skip_host:
        result["host_spsolve"] = host_baseline(problem(args.poses, args.loops, 100), args.iters)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "pose_graph_bench.json"), "w") as f:
        json.dump(result, f, indent=1)
    lines = ["# Pose-graph backend: one `optimize` replay", "",
             "`python tools/pose_graph_bench.py` on one MI355X; the data is `pose_graph_bench.json`.  N = %d poses, %d loops, %d "
             "LM iterations, %d alternated repeats, median (min - max).  No time against the reference exists: g2o is not "
             "installed." % (args.poses, args.loops, args.iters, args.repeats), "",
             "| streams | one replay | CG iterations per LM step (stream 0) | final relative residual (stream 0) | hit pcg_iters |",
             "|---|---|---|---|---|"]
    for S in args.streams:
        d = result["device"][str(S)]
        lines.append("| %d | %.1f ms (%.1f - %.1f) | %s | %s | %s |" % (
            S, d["ms_median"], d["ms_min"], d["ms_max"], d["pcg_used"][0],
            ["%.1e" % v for v in d["relres"][0]], "yes (%d)" % d["pcg_iters"] if d["hit_pcg_iters"] else "no"))
    if "host_spsolve" in result:
        h = result["host_spsolve"]
        lines += ["", "Host baseline, the model's LM with `scipy.sparse.linalg.spsolve` (%d CPUs visible): %.2f s for %d LM steps, "
                  "chi2 %.6g." % (h["threads"], h["seconds"], h["lm_steps"], h["chi2"])]
    with open(os.path.join(args.out, "README.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps({k: v for k, v in result.items() if k != "device"} |
                     {"device_ms": {S: result["device"][str(S)]["ms_median"] for S in args.streams}}))


if __name__ == "__main__":
    main()
