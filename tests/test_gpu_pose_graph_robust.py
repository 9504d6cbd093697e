"""GPU tests of the robust kernels on the pose graph against the float64 model."""
import copy

import numpy as np
import pytest
import torch

import pose_graph_cases as pgc
import pose_graph_device as pgd
import pose_graph_model as pgm
import pose_graph_robust_cases as prc
import pose_graph_robust_model as prm

pytestmark = pytest.mark.gpu

KERNELS = ("huber", "geman_mcclure", "dcs")
EVERY_CLASS = ("chain", "loop", "absolute")


def same(a, b):
    """Equal to the bit where a number is meant; a NaN matches a NaN (its sign and payload are the processor's)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def device(g, rb, **kw):
    """The model graph in stream 0 of a PoseGraph.  The host refuses a measurement that is not finite, so such a loop is added
    with the identity and its measurement, like vertices moved after the append, is then written into the device buffer."""
    h = copy.deepcopy(g)
    h.loops = [(i, j, Z if np.all(np.isfinite(Z)) else np.eye(4), Om) for i, j, Z, Om in g.loops]
    kw.setdefault("graph", False)
    pg = pgd.make([h], robust=None if rb is None else rb.settings(), **kw)
    pg.bufs["X"][:g.n, 0].copy_(torch.from_numpy(g.X))
    for l, loop in enumerate(g.loops):
        pg.bufs["loop_Z"][0, l].copy_(torch.from_numpy(loop[2]))
    return pg


def check_linearise(name, g, rb):
    pg = device(g, rb)
    pg.bufs["slots"].fill_(7.5)                                       # whatever a launch does not write keeps this
    pg.linearise()
    pg.bufs["Xt"].copy_(pg.bufs["X"])
    pg.linearise(trial=True)
    dev, chi_only = pg.bufs["slots"][0].cpu().numpy(), pg.bufs["chi_new"][0].cpu().numpy()
    ref, (ids, vi, vj, ab) = prm.linearise(g, rb)
    _, _, _, Z, Om, _ = g.edges()
    assert same(dev[ids][:, pgm.CHI], ref[ids][:, pgm.CHI]), "rho"     # to the bit: the source order is the model's
    assert same(dev[ids][:, prm.RAW], ref[ids][:, prm.RAW]) and same(dev[ids][:, prm.W], ref[ids][:, prm.W]), "c, w"
    assert same(chi_only[ids], prm.chi_terms(g, rb, g.X)[ids]), "the chi-only pass"
    assert np.all(dev[ids][:, 135] == 7.5)
    other = np.ones(len(dev), bool); other[ids] = False
    assert np.all(dev[other] == 7.5) and not chi_only[other].any()    # ids that are no edge are never written
    # section 25's 1e-12 sum |term| on the plain blocks (the terms of an error are bounded by the translations it combines,
    # those of a block by |J|^T |Omega| |J| with |J| <= 1 + 2 |t_A|), carried through the one multiplication by w: w times the
    # plain bound, and one rounding of the product on either side
    w = ref[ids][:, prm.W]
    finite = np.isfinite(ref[ids]).all(1) & np.isfinite(w)
    with np.errstate(invalid="ignore"):
        tsum = 3.0 + np.abs(g.X[vi][:, :3, 3]).sum(1) + np.abs(g.X[vj][:, :3, 3]).sum(1) + np.abs(Z[:, :3, 3]).sum(1)
    jmax = 1.0 + 2.0 * tsum
    osum = np.abs(Om).sum((1, 2))
    tol = np.zeros((len(ids), pgm.SLOT))
    tol[:, pgm.E_:pgm.E_ + 6] = 1e-12 * tsum[:, None]
    tol[:, pgm.OE:pgm.OE + 6] = 1e-12 * (osum * tsum)[:, None]
    tol[:, pgm.HII:pgm.BI] = 1e-12 * (w * osum * jmax * jmax)[:, None]
    tol[:, pgm.BI:pgm.CHI] = 1e-12 * (w * osum * jmax * tsum)[:, None]
    tol[:, pgm.HII:pgm.CHI] += 2.0 * np.finfo(np.float64).eps * np.abs(np.where(np.isfinite(ref[ids]), ref[ids], 0.0))[:, pgm.HII:pgm.CHI]
    cols = np.r_[pgm.E_:pgm.CHI]
    written = np.ones((len(ids), pgm.SLOT), bool)
    written[np.ix_(ab, np.r_[pgm.HII:pgm.HJJ, pgm.BI:pgm.BJ])] = False   # the i side of an absolute edge
    assert np.all(dev[ids][~written] == 7.5)
    err = np.abs(dev[ids] - np.where(written, ref[ids], 7.5))[finite][:, cols]
    print("%s: worst block error / bound %.3g, weights %s" % (name, (err / np.maximum(tol[finite][:, cols], 1e-300)).max()
                                                             if finite.any() else 0.0, np.round(w[-4:], 4).tolist()))
    assert np.all(err <= tol[finite][:, cols])
    assert not np.isfinite(dev[ids][~finite][:, pgm.CHI]).any()        # a non-finite c stays visible to the solve
    return pg


@pytest.mark.parametrize("name", list(prc.TABLE))
def test_robust_linearise_on_the_edge_table(name):
    build, rb = prc.TABLE[name]
    with np.errstate(invalid="ignore"):
        check_linearise(name, build(), rb)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", ["n3", "n63", "n64", "n65", "three_share_a_vertex", "absolute_and_loop", "full_omega"])
def test_robust_linearise_on_the_graph_cases(name, kernel):
    """The cases of section 25 with the kernel on every class.  The vertices are moved off the chain first (a seeded
    perturbation of a few centimetres), so that the chain edges carry an error too."""
    g = pgc.CASES[name]()
    rng = np.random.default_rng(5)
    g.X[1:] = pgm.retract(g.X[1:], rng.normal(0.0, 0.05, (g.n - 1, 6)))
    check_linearise("%s %s" % (name, kernel), g, prm.Robust(kernel, 0.05, EVERY_CLASS))


def test_plain_launch_leaves_the_spare_doubles():
    build, rb = prc.TABLE["huber_on_chain_loop_absolute"]
    g = build()
    pg = device(g, None)
    pg.bufs["slots"].fill_(7.5)
    pg.linearise()
    dev = pg.bufs["slots"][0].cpu().numpy()
    ids = g.edges()[0]
    assert np.all(dev[:, 133:136] == 7.5) and np.array_equal(dev[ids][:, pgm.CHI], pgm.linearise(g)[0][ids][:, pgm.CHI])
    pg.set_robust(rb.settings())
    pg.linearise()
    dev = pg.bufs["slots"][0].cpu().numpy()
    assert np.all(dev[ids][:, 133:135] != 7.5) and np.all(dev[:, 135] == 7.5)


def test_library_refuses_bad_settings():
    build, rb = prc.TABLE["huber_c_1"]
    pg = device(build(), rb)
    before = pgd.snapshot(pg)
    for bad, word in (((1, 0.0, 2), "delta"), ((1, -1.0, 2), "delta"), ((1, float("inf"), 2), "delta"),
                      ((1, float("nan"), 2), "delta"), ((4, 1.0, 2), "kind"), ((0, 1.0, 2), "kind"), ((1, 1.0, 0), "edge_mask"),
                      ((1, 1.0, 8), "edge_mask")):
        pg._robust = bad
        for launch in (pg.linearise, lambda: pg.linearise(trial=True)) + ((pg.edge_weights,) if bad[0] else ()):
            with pytest.raises(RuntimeError, match=word):
                launch()
    after = pgd.snapshot(pg)
    assert all(torch.equal(after[k], before[k]) for k in before)       # refused before any launch


# ---- the read-out ------------------------------------------------------------------------------------------------------------

def _weights_graph(seed, ML, MA, nloops, nabs):
    g, gt = pgc.noisy_chain(64, seed, N=64, ML=ML, MA=MA)
    for l in range(nloops):
        i, j = l % 20, 30 + (l * 7) % 34
        g.add_loop(i, j, pgc.between(gt, i, j), prc.SCENE_OMEGA if l % 3 else None)
    for a in range(nabs):
        g.add_absolute((a * 5) % 64, gt[(a * 5) % 64] @ pgm.pose([0, 1, 0], 0.01 * a, [0.1 * a, 0.0, 0.0]))
    return g


@pytest.mark.parametrize("robust", [None, prm.Robust("geman_mcclure", 1.0), prm.Robust("huber", 0.05, EVERY_CLASS),
                                    prm.Robust("dcs", 0.5, ("absolute",))], ids=["none", "gm_loops", "huber_all", "dcs_abs"])
@pytest.mark.parametrize("ML,MA", [(40, 23), (40, 24), (40, 25)])      # 63, 64 and 65 ids: one workgroup, exactly one, two
def test_edge_weights_to_the_bit(ML, MA, robust):
    """S = 3 with full, few and no loops; stream 1 idles through an optimisation that moves the other two: the read-out runs
    for all three, whatever their status words say, at the vertices as they stand."""
    graphs = [_weights_graph(41, ML, MA, ML, MA), _weights_graph(42, ML, MA, 3, 1), _weights_graph(43, ML, MA, 0, 2)]
    pg = pgd.make(graphs, graph=False, iters=3, robust=None if robust is None else robust.settings())
    pg.optimize(active=torch.tensor([1, 0, 1], dtype=torch.int32).cuda())
    before = pgd.snapshot(pg)
    loops, absolutes = pg.edge_weights()
    assert loops.shape == (3, ML, 2) and absolutes.shape == (3, MA, 2)
    X = pg.bufs["X"].cpu().numpy()
    for s, g in enumerate(graphs):
        want = prm.edge_weights(g, robust, X[:g.n, s])
        got = torch.cat([loops[s], absolutes[s]]).cpu().numpy()
        assert np.array_equal(got, want), s
        assert np.array_equal(pg.loop_weights(s).cpu().numpy(), want[:len(g.loops)])
        one = pg.edge_weights(stream=s)
        assert torch.equal(one[0], loops[s]) and torch.equal(one[1], absolutes[s])
        if robust is None:
            assert np.all(want[:len(g.loops), 1] == 1.0)
    after = pgd.snapshot(pg)
    assert all(torch.equal(after[k], before[k]) for k in before if k != "weights")   # a read-out: nothing else moves


# ---- whole optimisations ---------------------------------------------------------------------------------------------------------

def test_scene_optimize_rejects_the_false_loop():
    """The scene at N = 64, 20 iterations, Geman-McClure with delta = 1 on the loops.  Yardstick as in section 25: the
    distance between the model's dense and the model's own CG result; the device must lie within 4 x of the dense result.
    Status equals the CG model's.  chi2 against the CG model: the sum of some 65 non-negative terms, each within section 25's
    1e-12 of itself, so 1e-12 chi2 (at a minimum the poses' own difference enters only in second order)."""
    rb = prc.SCENE_ROBUST
    a, b, c = prc.scene(N=64)[0], prc.scene(N=64)[0], prc.scene(N=64)[0]
    start = c.X.copy()
    ra, rb_ = prm.optimize(a, rb, iters=20, solver="dense"), prm.optimize(b, rb, iters=20, solver="cg")
    yt, yr = pgm.distance(a.X, b.X)

    def run(graph):
        pg = device(c, rb, graph=graph, iters=20)
        keep = {k: pg.bufs[k].clone() for k in ("X", "lam", "nu", "chi2", "status")}
        out = []
        for _ in range(3):                                            # eager, then the capture and a replay
            for k, v in keep.items():
                pg.bufs[k].copy_(v)
            pg.optimize()
            out.append({k: pg.bufs[k].clone() for k in ("X", "lam", "chi2", "status", "accepted", "pcg_used")})
        return pg, out
    pg, replayed = run(True)
    pe, eager = run(False)
    assert pg.captures == 1 and pe.captures == 0
    for x in replayed[1:] + eager:
        assert all(torch.equal(x[k], replayed[0][k]) for k in x)      # eager equals replay, bit for bit
    X = pg.poses(0).cpu().numpy()
    dt, dr = pgm.distance(a.X, X)
    chi2, w = float(pg.chi2()[0]), pg.loop_weights(0).cpu().numpy()
    print("yardstick (dense vs CG model) %.3g m %.3g rad; device vs dense %.3g m %.3g rad; chi2 device %.17g CG model %.17g "
          "dense %.17g; status %d / %d; moved %.3g m from the odometry; weights %s; pcg %s"
          % (yt, yr, dt, dr, chi2, rb_["chi2"], ra["chi2"], int(pg.status()[0]), rb_["status"], pgm.distance(start, X)[0],
             w[:, 1].tolist(), pg.bufs["pcg_used"][0].tolist()))
    assert int(pg.status()[0]) == rb_["status"]
    assert abs(chi2 - rb_["chi2"]) <= 1e-12 * rb_["chi2"]
    assert dt <= 4.0 * yt and dr <= 4.0 * yr
    assert np.all(w[5, 1] < w[:5, 1]) and np.array_equal(w, prm.edge_weights(c, rb, X)[:6])
    # another setting after the capture is honoured by a new capture, never ignored
    pg.bufs["X"][:c.n, 0].copy_(torch.from_numpy(start))
    pg.set_robust(None)
    pg.optimize()
    plain = device(c, None, iters=20)
    plain.optimize()
    assert pg.captures == 2 and torch.equal(pg.poses(0), plain.poses(0)) and not torch.equal(pg.poses(0), replayed[0]["X"][:c.n, 0])


def test_no_kernel_keeps_the_bits_of_one_loop():
    """``robust=None`` takes the plain launches (their slots' spare doubles stay zero), and a kernel that never engages (Huber
    with delta = 1e150: rho = c, w = 1 on every edge) takes the robust ones to the same bits."""
    g = pgc.CASES["one_loop"]()
    pa, pb = device(g, None), device(g, prm.Robust("huber", 1e150, EVERY_CLASS))
    pc = pgd.make([pgc.CASES["one_loop"]()], graph=False)              # as the tests of section 25 build it
    for p in (pa, pb, pc):
        p.optimize()
    for k in ("X", "Xt", "lam", "nu", "chi2", "status", "delta", "chi_new", "accepted", "pcg_used", "relres"):
        assert torch.equal(pa.bufs[k], pb.bufs[k]) and torch.equal(pa.bufs[k], pc.bufs[k]), k
    assert torch.equal(pa.bufs["slots"], pc.bufs["slots"]) and not pa.bufs["slots"][:, :, 133:].any()
    assert torch.equal(pa.bufs["slots"][:, :, :133], pb.bufs["slots"][:, :, :133])
    assert int(pa.bufs["accepted"][0].sum()) >= 1                      # (something was optimised)


def test_non_finite_term_still_sets_the_status_bit():
    build, rb = prc.TABLE["geman_mcclure_c_not_finite"]
    with np.errstate(invalid="ignore"):
        pg = device(build(), rb)
    pg.optimize()
    assert int(pg.status()[0]) == pgm.NONFINITE


def test_graph_slam_robust_kernel_on_the_device():
    from pwclonet_pylidarslam_amd.backend import GraphSLAM, GraphSLAMConfig, RobustKernel
    g, _ = prc.scene(N=64)
    slam = GraphSLAM(GraphSLAMConfig(max_poses=64, max_loops=8, max_absolute=8, max_optim_iterations=20, online_optimization=False))
    slam.robust_kernel = RobustKernel("geman_mcclure", 1.0)           # before init(): the graph is made with it
    slam.init()
    for k in range(1, g.n):
        frame = {GraphSLAM.se3_odometry_constraint(k - 1): (g.Z[k], None)}
        if k == g.n - 1:
            for i, j, Z, Om in g.loops:
                frame[GraphSLAM.se3_loop_closure_constraint(i, j)] = (Z, Om)
        slam.next_frame(frame)
    rb = prm.Robust("geman_mcclure", 1.0, EVERY_CLASS)
    pg = device(g, rb, iters=20)
    pg.optimize()
    assert np.array_equal(slam.world_poses(), pg.poses(0).cpu().numpy())
    w = slam.pose_graph().loop_weights(0)[:, 1]
    assert bool((w[5] < w[:5]).all())
    slam.robust_kernel = None                                          # acts on every edge at the next optimize
    assert slam.pose_graph().robust() is None


def test_streaming_backend_passes_the_kernel_through(cuda):
    from test_gpu_pose_graph_stream import BACKEND, REFINE, _net
    import icp_mask_model as masked
    from pwclonet_pylidarslam_amd import synthetic
    from pwclonet_pylidarslam_amd.odometry import StreamingOdometry
    from pwclonet_pylidarslam_amd.pose_graph import PoseGraph
    S, n, F = 2, masked.N, 6
    robust = dict(kernel="geman_mcclure", delta=0.01)
    seqs = [synthetic.kitti_like_sequence(31 + i, n, F)[0] for i in range(S)]
    so = StreamingOdometry(_net(cuda), streams=S, max_frames=8, refine=dict(REFINE), backend=dict(BACKEND, robust=robust))
    with torch.no_grad():
        for f in range(F):
            so.step(torch.from_numpy(np.stack([seqs[s][f] for s in range(S)])).to(cuda))
    pg = so.backend()
    assert pg.robust() == (2, 0.01, 2)
    Z = pgm.pose([0, 0, 1], 0.02, [0.3, 0.1, 0.0])
    chain = so.refined_relative_poses()
    alone, plain = PoseGraph(S, max_poses=8, robust=robust, **BACKEND), PoseGraph(S, max_poses=8, **BACKEND)
    for p in (alone, plain):
        for k in range(1, F):
            p.append(chain[k].contiguous())
    for p in (pg, alone, plain):
        p.add_loop(1, 0, F - 1, Z)
        p.optimize()
    got = so.optimized_trajectory()
    assert torch.equal(got, alone.poses()) and not torch.equal(got, plain.poses())
    w = pg.loop_weights(1)
    assert torch.equal(w, alone.loop_weights(1)) and 0.0 < float(w[0, 1]) < 1.0 and pg.loop_weights(0).shape == (0, 2)
