"""GPU tests of the pose-graph backend at its edges: refusals, overflow, idle streams beside poisoned buffers, reset, priming
on the device."""
import numpy as np
import pytest
import torch

import pose_graph_cases as pgc
import pose_graph_device as pgd
import pose_graph_model as pgm

pytestmark = pytest.mark.gpu


def _graph(n=12, seed=31, **kw):
    g, gt = pgc.noisy_chain(n, seed, **kw)
    g.add_loop(1, n - 2, pgc.between(gt, 1, n - 2))
    return g, gt


def test_python_refusals_write_nothing():
    from pwclonet_pylidarslam_amd.pose_graph import PoseGraph
    for kw in (dict(streams=1025), dict(streams=0), dict(streams=1, max_poses=0), dict(streams=1, max_loops=0),
               dict(streams=1, max_absolute=-1), dict(streams=1, iters=0), dict(streams=1, pcg_tol=1.0)):
        with pytest.raises(ValueError):
            PoseGraph(**kw)
    g, gt = _graph()
    pg = pgd.make([g], graph=False)
    before = pgd.snapshot(pg)
    bad_om = np.eye(6); bad_om[0, 1] = 0.5
    nan_om = np.eye(6); nan_om[2, 2] = np.nan
    T = np.eye(4)
    for call in (lambda: pg.add_loop(0, 5, 5, T), lambda: pg.add_loop(0, 7, 3, T), lambda: pg.add_loop(0, 2, 12, T),
                 lambda: pg.add_loop(0, -1, 4, T), lambda: pg.add_loop(1, 1, 4, T), lambda: pg.add_loop(0, 1, 4, T, bad_om),
                 lambda: pg.add_loop(0, 1, 4, T, nan_om), lambda: pg.add_absolute(0, 12, T),
                 lambda: pg.add_absolute(0, 3, T, bad_om), lambda: pg.add_loop(0, 1, 4, np.full((4, 4), np.inf))):
        with pytest.raises(ValueError):
            call()
    after = pgd.snapshot(pg)
    for k in before:
        assert torch.equal(before[k], after[k]), k


def test_library_refusals_launch_nothing():
    """The C entries refuse S > 1024 and capacities <= 0 before any launch: the sentinel bytes stay."""
    from pwclonet_pylidarslam_amd import _lib
    from pwclonet_pylidarslam_amd.registration import _p
    g, _ = _graph()
    pg = pgd.make([g], graph=False)
    b = pg.bufs
    b["slots"].fill_(-7.0); b["Xt"].fill_(-7.0); b["delta"].fill_(-7.0)
    before = pgd.snapshot(pg)
    lin = lambda S, N, ML, MA: _lib.call(
        "pose_graph_linearise_kernel_wrapper", pg.device, S, N, ML, MA, _p(b["active"]), _p(b["status"]), _p(b["count"]),
        _p(b["nloops"]), _p(b["nabs"]), _p(b["X"]), _p(b["Zc"]), _p(b["loop_ij"]), _p(b["loop_Z"]), _p(b["loop_Om"]),
        _p(b["abs_i"]), _p(b["abs_G"]), _p(b["abs_Om"]), _p(b["slots"]), 0)
    app = lambda S, N: _lib.call(
        "pose_graph_append_kernel_wrapper", pg.device, S, N, 0, 0, 0, _p(b["Xt"]), 0, _p(b["X"]), _p(b["Zc"]), _p(b["count"]),
        _p(b["nloops"]), _p(b["nabs"]), _p(b["epoch"]), _p(b["overflow"]))
    ret = lambda S, N: _lib.call("pose_graph_retract_kernel_wrapper", pg.device, S, N, 1, 0, _p(b["status"]), _p(b["count"]),
                                 _p(b["X"]), _p(b["delta"]), _p(b["Xt"]))
    for call in (lambda: lin(1025, 12, 8, 8), lambda: lin(0, 12, 8, 8), lambda: lin(1, 0, 8, 8), lambda: lin(1, 12, 0, 8),
                 lambda: lin(1, 12, 8, -1), lambda: app(1025, 12), lambda: app(1, 0), lambda: ret(1025, 12), lambda: ret(1, 0)):
        with pytest.raises(RuntimeError):
            call()
    after = pgd.snapshot(pg)
    for k in before:
        assert torch.equal(before[k], after[k]), k


def test_overflow_word_and_nothing_written():
    from pwclonet_pylidarslam_amd.pose_graph import PoseGraph
    pg = PoseGraph(2, max_poses=4, max_loops=1, max_absolute=1, graph=False)
    rel = torch.from_numpy(np.stack([pgm.pose([0, 0, 1], 0.1, [1, 0, 0])] * 2)).cuda()
    for _ in range(3):
        pg.append(rel)
    assert not pg.overflowed() and pg.counts().tolist() == [4, 4]
    before = pgd.snapshot(pg)
    pg.append(rel, active=torch.tensor([0, 1], dtype=torch.int32).cuda())        # vertex max_poses + 1 of stream 1
    after = pgd.snapshot(pg)
    assert pg.overflowed()
    for k in before:
        if k != "overflow":
            assert torch.equal(before[k], after[k]), k


def test_idle_streams_keep_every_bit_beside_poison():
    graphs = [_graph(12, 40 + s, N=16)[0] for s in range(3)]
    pg = pgd.make(graphs, graph=False, iters=4)
    pg.optimize()                                                     # every stream has lambda, status, slots of its own
    for k in ("slots", "chi_new", "delta", "Xt"):                      # poison what an idle stream must not touch
        pg.bufs[k][..., 1, :, :].fill_(float("nan")) if k == "Xt" else pg.bufs[k][1].fill_(float("nan"))
    before = pgd.snapshot(pg)
    act = torch.tensor([1, 0, 1], dtype=torch.int32).cuda()
    pg.append(torch.from_numpy(np.stack([pgm.pose([0, 0, 1], 0.05, [1, 0, 0])] * 3)).cuda(), active=act)
    pg.optimize(active=act)
    after = pgd.snapshot(pg)
    for k in ("X", "Xt", "Zc"):
        assert torch.equal(after[k][:, 1].view(torch.int64), before[k][:, 1].view(torch.int64)), k
    for k in ("count", "lam", "nu", "chi2", "status", "slots", "chi_new", "delta", "nloops", "loop_ij", "loop_Z", "loop_Om",
              "pcg_used", "relres", "accepted", "inc_ptr", "inc_ent"):
        a, c = after[k][1], before[k][1]
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                           c.view(torch.int64) if c.dtype == torch.float64 else c), k
    assert pg.counts().tolist() == [13, 12, 13] and not torch.equal(after["X"][:12, 0], before["X"][:12, 0])


def test_reset_one_stream_and_prime_on_device():
    graphs = [_graph(12, 50 + s, N=16)[0] for s in range(3)]
    pg = pgd.make(graphs, graph=False, iters=3)
    before = pgd.snapshot(pg)
    pg.reset(streams=[1])
    after = pgd.snapshot(pg)
    assert pg.counts().tolist() == [12, 1, 12] and after["nloops"].tolist() == [1, 0, 1]
    for s in (0, 2):
        assert torch.equal(after["X"][:, s], before["X"][:, s]) and torch.equal(after["loop_Z"][s], before["loop_Z"][s])
    pg.optimize()
    assert int(pg.status()[1]) == pgm.CONVERGED | pgm.TRIVIAL
    # a prime on the device (active and not valid) empties stream 2 alone; the host notices at its next add_*
    rel = torch.from_numpy(np.stack([pgm.pose([0, 0, 1], 0.05, [1, 0, 0])] * 3)).cuda()
    pg.append(rel, valid=torch.tensor([1, 1, 0], dtype=torch.int32).cuda())
    assert pg.counts().tolist() == [13, 2, 1] and pg.bufs["nloops"].tolist() == [1, 0, 0]
    with pytest.raises(ValueError):
        pg.add_loop(2, 0, 5, np.eye(4))                               # stream 2 holds one pose now
    pg.append(rel); pg.append(rel)
    pg.add_loop(2, 0, 2, np.eye(4))
    assert pg.bufs["nloops"].tolist() == [1, 0, 1] and pg.bufs["loop_ij"][2, 0].tolist() == [0, 2]
    pg.optimize()
    assert int(pg.status()[2]) & pgm.TRIVIAL == 0 and int(pg.bufs["accepted"][2, 0]) == 1     # the new graph is optimised
    assert 0.0 < float(pg.chi2()[2]) < float("inf")


def test_non_finite_input_freezes_the_stream():
    graphs = [_graph(12, 60 + s, N=16)[0] for s in range(2)]
    pg = pgd.make(graphs, graph=False, iters=3)
    pg.bufs["loop_Z"][1, 0, 0, 3] = float("nan")
    before = pgd.snapshot(pg)
    pg.optimize()
    assert int(pg.status()[1]) == pgm.NONFINITE and torch.equal(pg.bufs["X"][:, 1], before["X"][:, 1])
    assert int(pg.status()[0]) != pgm.NONFINITE and not torch.equal(pg.bufs["X"][:, 0], before["X"][:, 0])


def test_rows_input_matches_matrices():
    from pwclonet_pylidarslam_amd.pose_graph import PoseGraph
    rows = torch.tensor([[0.5, -0.25, 0.125, 0.9689124217106447, 0.0, 0.0, 0.24740395925452294]], dtype=torch.float32).cuda()
    a, b = PoseGraph(1, 4, 1, 1), PoseGraph(1, 4, 1, 1)
    a.append(rows)
    r = rows[0].double().cpu().numpy()
    w, x, y, z = r[3:]
    s = 2.0 / (w * w + x * x + y * y + z * z)
    R = np.array([[1 - s * (y * y + z * z), s * (x * y - w * z), s * (x * z + w * y)],
                  [s * (x * y + w * z), 1 - s * (x * x + z * z), s * (y * z - w * x)],
                  [s * (x * z - w * y), s * (y * z + w * x), 1 - s * (x * x + y * y)]])
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = r[:3]
    b.append(torch.from_numpy(T)[None].cuda())
    assert np.abs(a.poses(0).cpu().numpy() - b.poses(0).cpu().numpy()).max() <= 1e-15


def test_default_information_on_the_device():
    """add_loop / add_absolute without an information matrix: what reaches the device on either side of |i - j| = 4."""
    g, gt = pgc.noisy_chain(12, 81, N=16)
    pg = pgd.make([g], graph=False)
    pg.add_loop(0, 2, 6, pgc.between(gt, 2, 6))
    pg.add_loop(0, 2, 7, pgc.between(gt, 2, 7))
    pg.add_loop(0, 0, 11, pgc.between(gt, 0, 11))
    pg.add_absolute(0, 3, gt[3])
    om = pg.bufs["loop_Om"][0].cpu().numpy()
    assert np.array_equal(om[0], np.diag([2.0, 2, 2, 5, 5, 5])) and np.array_equal(om[1], np.diag([.1, .1, .1, .5, .5, .5]))
    assert np.array_equal(om[2], np.diag([.1, .1, .1, .5, .5, .5]))
    assert np.array_equal(pg.bufs["abs_Om"][0, 0].cpu().numpy(), np.diag([1.0, 1, 1, .001, .001, .001]))
    for i, j in ((2, 6), (2, 7), (0, 11)):
        g.add_loop(i, j, pgc.between(gt, i, j))
    g.add_absolute(3, gt[3])
    pg.linearise()
    ref, (ids, _, _, _) = pgm.linearise(g)
    assert np.array_equal(pg.bufs["slots"][0].cpu().numpy()[ids][:, pgm.CHI], ref[ids][:, pgm.CHI])


def test_library_refusals_of_begin_solve_and_judge():
    from pwclonet_pylidarslam_amd import _lib
    from pwclonet_pylidarslam_amd.registration import _p
    g, _ = _graph()
    pg = pgd.make([g], graph=False, iters=4)
    b = pg.bufs
    pg.linearise()
    for k in ("delta", "Xt", "chi_new"):
        b[k].fill_(-7.0)
    before = pgd.snapshot(pg)

    def solve(S=1, N=12, ML=8, MA=8, it=0, pcg_iters=10, tol=1e-8, stride=4):
        _lib.call("pose_graph_solve_kernel_wrapper", pg.device, S, N, ML, MA, 1, it, pcg_iters, tol, _p(b["active"]),
                  _p(b["status"]), _p(b["count"]), _p(b["nloops"]), _p(b["nabs"]), _p(b["loop_ij"]), _p(b["abs_i"]),
                  _p(b["inc_ptr"]), _p(b["inc_ent"]), _p(b["slots"]), _p(b["X"]), _p(b["work"]), _p(b["delta"]), _p(b["Xt"]),
                  _p(b["lam"]), _p(b["nu"]), _p(b["chi2"]), _p(b["pcg_used"]), _p(b["relres"]), stride)

    def judge(S=1, N=12, ML=8, MA=8, it=0, stride=4):
        _lib.call("pose_graph_judge_kernel_wrapper", pg.device, S, N, ML, MA, 1, it, _p(b["active"]), _p(b["status"]),
                  _p(b["count"]), _p(b["nloops"]), _p(b["nabs"]), _p(b["loop_ij"]), _p(b["abs_i"]), _p(b["inc_ptr"]),
                  _p(b["inc_ent"]), _p(b["slots"]), _p(b["chi_new"]), _p(b["delta"]), _p(b["Xt"]), _p(b["X"]), _p(b["lam"]),
                  _p(b["nu"]), _p(b["chi2"]), _p(b["accepted"]), stride)

    def begin(S=1, iters=4, stride=4):
        _lib.call("pose_graph_begin_kernel_wrapper", pg.device, S, iters, stride, _p(b["active"]), _p(b["count"]),
                  _p(b["nloops"]), _p(b["nabs"]), _p(b["status"]), _p(b["pcg_used"]), _p(b["relres"]), _p(b["accepted"]),
                  _p(b["chi2"]))
    calls = [lambda: solve(S=1025), lambda: solve(S=0), lambda: solve(N=0), lambda: solve(ML=0), lambda: solve(MA=-3),
             lambda: solve(it=4), lambda: solve(it=-1), lambda: solve(pcg_iters=0), lambda: solve(tol=1.0),
             lambda: solve(tol=-1e-3), lambda: judge(S=1025), lambda: judge(N=0), lambda: judge(ML=0), lambda: judge(MA=0),
             lambda: judge(it=4), lambda: judge(it=-1), lambda: begin(S=1025), lambda: begin(S=0), lambda: begin(iters=0),
             lambda: begin(iters=5)]
    for k, call in enumerate(calls):
        with pytest.raises(RuntimeError):
            call()
    after = pgd.snapshot(pg)
    for k in before:
        assert torch.equal(before[k], after[k]), k
