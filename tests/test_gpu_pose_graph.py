"""GPU tests of the pose-graph kernels against the float64 model."""
import numpy as np
import pytest
import torch

import pose_graph_cases as pgc
import pose_graph_device as pgd
import pose_graph_model as pgm

pytestmark = pytest.mark.gpu


def _same_capacity(name, N):
    g = pgc.CASES[name]()
    g.N = N
    return g


@pytest.mark.parametrize("name", list(pgc.CASES))
def test_linearise_matches_model(name):
    g = pgc.CASES[name]()
    pg = pgd.make([g], graph=False)
    assert int(pg.counts()[0]) == g.n and torch.equal(pg.poses(0).cpu(), torch.from_numpy(g.X))   # the append's products
    pg.linearise()
    dev = pg.bufs["slots"][0].cpu().numpy()
    ref, (ids, vi, vj, ab) = pgm.linearise(g)
    if not len(ids):
        assert not dev.any()
        return
    _, _, _, Z, Om, _ = g.edges()
    # 1e-12 sum |term|: the terms of an error are bounded by the translations it combines (rotation entries are <= 1), the
    # terms of a block by |J|^T |Omega| |J| with |J| <= 1 + 2 |t_A|
    tsum = 3.0 + np.abs(g.X[vi][:, :3, 3]).sum(1) + np.abs(g.X[vj][:, :3, 3]).sum(1) + np.abs(Z[:, :3, 3]).sum(1)
    jmax = 1.0 + 2.0 * tsum
    osum = np.abs(Om).sum((1, 2))
    tol = np.zeros((len(ids), pgm.SLOT))
    tol[:, pgm.E_:pgm.E_ + 6] = 1e-12 * tsum[:, None]
    tol[:, pgm.OE:pgm.OE + 6] = 1e-12 * (osum * tsum)[:, None]
    tol[:, pgm.HII:pgm.BI] = 1e-12 * (osum * jmax * jmax)[:, None]
    tol[:, pgm.BI:pgm.CHI] = 1e-12 * (osum * jmax * tsum)[:, None]
    tol[:, pgm.CHI] = 1e-12 * osum * tsum * tsum
    err = np.abs(dev[ids] - ref[ids])
    print("%s: worst error / bound %.3g" % (name, (err / np.maximum(tol, 1e-300)).max()))
    assert np.all(err <= tol)
    mask = np.ones(len(dev), bool); mask[ids] = False
    assert not dev[mask].any()                                       # ids that are no edge are never written
    assert np.array_equal(dev[ids][:, pgm.CHI], ref[ids][:, pgm.CHI])   # the chi2 terms agree to the bit (source order)


@pytest.mark.parametrize("name", pgc.OPTIMISED)
def test_solve_teacher_forced(name):
    g = pgc.CASES[name]()
    pg = pgd.make([g], graph=False)
    slots, table = pgm.linearise(g)
    H, b = pgm.assemble(g, slots, table)
    idx = pgm.free_index(g)
    lam = 1e-5 * np.max(np.diag(H)[idx])
    pg.linearise()
    pg.bufs["lam"].fill_(lam)
    pg.solve(it=1)                                                   # it > 0: lambda is taken as given
    d = pg.bufs["delta"][0, :g.n].cpu().numpy().reshape(-1)
    res = np.linalg.norm((H[np.ix_(idx, idx)] + lam * np.eye(len(idx))) @ d[idx] + b[idx])
    used, rel = int(pg.bufs["pcg_used"][0, 1]), float(pg.bufs["relres"][0, 1])
    print("%s: true residual %.3g |b|, recurrence %.3g, %d iterations" % (name, res / np.linalg.norm(b[idx]), rel, used))
    assert 1 <= used <= pg.pcg_iters and rel <= 1e-8
    assert res <= 2.0 * 1e-8 * np.linalg.norm(b[idx])
    if g.fix_first:
        assert not d[:6].any()
    Xt = pg.bufs["Xt"][:g.n, 0].cpu().numpy()
    free = g.free()
    want = g.X.copy(); want[free] = pgm.retract(g.X[free], d.reshape(-1, 6)[free])
    assert np.array_equal(Xt, want)                                  # the retraction, bit for bit


@pytest.mark.parametrize("name", pgc.OPTIMISED)
@pytest.mark.parametrize("scale", [1.0, 40.0])                       # the model's step (accepted) and an overshoot (rejected)
def test_judge_teacher_forced(name, scale):
    g = pgc.CASES[name]()
    pg = pgd.make([g], graph=False)
    slots, table = pgm.linearise(g)
    H, b = pgm.assemble(g, slots, table)
    lam = 1e-5 * np.max(np.diag(H)[pgm.free_index(g)])
    delta = pgm.solve(g, H, b, lam)[0] * scale
    pg.linearise()
    pg.solve(it=0)                                                   # chi2 of the linearisation point
    dev_slots = pg.bufs["slots"][0].cpu().numpy()
    chi = float(pg.chi2()[0])
    assert chi == pgm.block_sum(dev_slots[:, pgm.CHI])
    pg.bufs["lam"].fill_(lam); pg.bufs["nu"].fill_(2.0)
    pg.bufs["delta"][0, :g.n].copy_(torch.from_numpy(delta))
    pg.retract(); pg.linearise(trial=True); pg.judge(it=0)
    want = pgm.judge(g, g.X, delta, pgm.gather_b(g, dev_slots), lam, 2.0, chi)
    print("%s x%g: rho %.6g accepted %s lambda %.17g" % (name, scale, want["rho"], want["accepted"], want["lam"]))
    assert bool(pg.bufs["accepted"][0, 0]) == want["accepted"]
    assert float(pg.bufs["lam"][0]) == want["lam"] and float(pg.bufs["nu"][0]) == want["nu"]
    assert int(pg.status()[0]) == want["status"] and float(pg.chi2()[0]) == want["chi"]
    assert np.array_equal(pg.poses(0).cpu().numpy(), want["X"])


def test_circle_whole_optimisation():
    """The yardstick is the distance between the model's dense and the model's CG result; the device must lie within 4 x of
    the dense result."""
    a, b, c = pgc.circle()[0], pgc.circle()[0], pgc.circle()[0]
    ra, rb = pgm.optimize(a, solver="dense"), pgm.optimize(b, solver="cg")
    yt, yr = pgm.distance(a.X, b.X)
    yc = abs(ra["chi2"] - rb["chi2"]) / ra["chi2"]
    pg = pgd.make([c])
    pg.optimize()
    X = pg.poses(0).cpu().numpy()
    dt, dr = pgm.distance(a.X, X)
    dc = abs(float(pg.chi2()[0]) - ra["chi2"]) / ra["chi2"]
    print("yardstick (dense vs CG model): %.3g m %.3g rad %.3g chi2; device vs dense: %.3g m %.3g rad %.3g chi2; ratios "
          "%.2f %.2f %.2f" % (yt, yr, yc, dt, dr, dc, dt / yt, dr / yr, dc / yc))
    print("pcg iterations per step", pg.bufs["pcg_used"][0].tolist())
    assert float(pg.chi2()[0]) * 100.0 < ra["chi2_0"] and np.linalg.norm(X[100, :3, 3]) < 1e-3
    assert dt <= 4.0 * yt and dr <= 4.0 * yr and dc <= 4.0 * yc


@pytest.mark.parametrize("name", ["n1", "n2", "no_loop"])
def test_trivial_chain_bit_for_bit(name):
    g = pgc.CASES[name]()
    pg = pgd.make([g], graph=False)
    before = pgd.snapshot(pg)
    pg.optimize()
    assert int(pg.status()[0]) == pgm.CONVERGED | pgm.TRIVIAL and float(pg.chi2()[0]) == 0.0
    for k in ("X", "Zc", "count", "lam", "nu"):
        assert torch.equal(pg.bufs[k], before[k]), k


@pytest.mark.parametrize("S,seed", [(2, 0), (33, 1)])
def test_streams_and_scattered_masks(S, seed):
    """Every stream holds another case; an optimisation under a scattered mask equals the single-stream runs bit for bit, and
    the idle streams keep every bit."""
    rng = np.random.default_rng(seed)
    names = [pgc.OPTIMISED[k % 11] if k % 5 else "no_loop" for k in range(S)]     # (n257 and the circle stay out: capacity)
    names = [{"n257": "n65", "absolute_on_0_free": "absolute_and_loop"}.get(n, n) for n in names]   # (one fix_first per object)
    graphs = [_same_capacity(n, 128) for n in names]
    pg = pgd.make(graphs, graph=False, iters=6)
    active = torch.from_numpy((rng.random(S) < 0.6).astype(np.int32))
    active[0] = 1
    if S > 1:
        active[1] = 0
    before = pgd.snapshot(pg)
    pg.optimize(active=active.cuda())
    after = pgd.snapshot(pg)
    for s in range(S):
        if not active[s]:
            for k in ("X", "Xt", "Zc"):
                assert torch.equal(after[k][:, s], before[k][:, s]), (s, k)
            for k in ("count", "lam", "nu", "chi2", "status", "slots", "delta", "loop_Z", "nloops"):
                assert torch.equal(after[k][s], before[k][s]), (s, k)
            continue
        one = pgd.make([_same_capacity(names[s], 128)], graph=False, iters=6)
        one.optimize()
        assert torch.equal(one.poses(0), pg.poses(s)), (s, names[s])
        assert torch.equal(one.bufs["lam"][0], after["lam"][s]) and int(one.status()[0]) == int(after["status"][s])


def test_run_to_run_graph_replay_and_late_loop():
    def run(graph):
        g, gt = pgc.noisy_chain(40, 21, ML=4, MA=2)
        g.add_loop(0, 30, pgc.between(gt, 0, 30))
        pg = pgd.make([g], graph=graph, iters=5)
        out = []
        pg.optimize(); out.append(pg.poses(0).clone())
        pg.optimize(); out.append(pg.poses(0).clone())
        pg.add_loop(0, 3, 39, pgc.between(gt, 3, 39))                 # after the capture
        pg.optimize(); out.append(pg.poses(0).clone())
        return pg, out
    pa, a = run(True)
    pb, b = run(True)
    pe, e = run(False)
    assert pa.captures == 1 and pe.captures == 0
    for x, y, z in zip(a, b, e):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert not torch.equal(a[1], a[2]) and int(pa.bufs["nloops"][0]) == 2      # the late loop moved the poses
