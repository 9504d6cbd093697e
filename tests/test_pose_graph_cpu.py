"""CPU tests of the pose-graph model and its tables: the analytic Jacobians against central
differences, the reference's circle problem, trivial chains, the conditioning the device residual bound rests on, and the
planted faults, each of which must change a table row."""
import numpy as np
import pytest

import pose_graph_cases as pgc
import pose_graph_model as pgm


def _edge(rng, delta):
    """Xi, Xj, Z with Z^-1 Xi^-1 Xj = delta."""
    Xi = pgm.pose(rng.normal(size=3), rng.uniform(0.2, 2.5), rng.normal(size=3))
    Z = pgm.pose(rng.normal(size=3), rng.uniform(0.2, 2.5), rng.normal(size=3))
    return Xi, Xi @ Z @ delta, Z


def _jacobian_cases():
    rng = np.random.default_rng(0)
    out = [("random%d" % k, pgm.pose(rng.normal(size=3), rng.uniform(0.1, 3.0), rng.normal(size=3))) for k in range(6)]
    for a, axis in enumerate(np.eye(3)):
        for deg in (179.9, 180.1):
            out.append(("%s%.1f" % ("xyz"[a], deg), pgm.pose(axis, np.radians(deg), rng.normal(size=3))))
    return out


def _numeric(Xi, Xj, Z, side, h=1e-6):
    Om, ab = np.eye(6)[None], np.array([False])
    J = np.zeros((6, 6))
    for c in range(6):
        e = []
        for sgn in (1.0, -1.0):
            d = np.zeros(6); d[c] = sgn * h
            a, b = (pgm.retract(Xi, d), Xj) if side == "i" else (Xi, pgm.retract(Xj, d))
            e.append(pgm.edge_error(a[None], b[None], Z[None], Om, ab)["e"][0])
        J[:, c] = (e[0] - e[1]) / (2 * h)
    return J


def _jacobian_error(faults=()):
    rng = np.random.default_rng(1)
    worst, branches, signs = 0.0, set(), set()
    for name, delta in _jacobian_cases():
        Xi, Xj, Z = _edge(rng, delta)
        err = pgm.edge_error(Xi[None], Xj[None], Z[None], np.eye(6)[None], np.array([False]))
        Ji, Jj = pgm.jacobians(err, Z[None], np.array([False]), faults)
        branches.add(int(err["branch"][0])); signs.add(float(err["sg"][0]))
        worst = max(worst, np.abs(Ji[0] - _numeric(Xi, Xj, Z, "i")).max(), np.abs(Jj[0] - _numeric(Xi, Xj, Z, "j")).max())
    return worst, branches, signs


def test_jacobians_against_central_differences():
    worst, branches, signs = _jacobian_error()
    print("max |analytic - numeric| = %.3g" % worst)
    assert branches == {0, 1, 2, 3} and signs == {-1.0, 1.0}       # every Shepperd branch, w on both sides of 0
    assert worst <= 1e-7


def test_absolute_edge_jacobian():
    rng = np.random.default_rng(2)
    G, X = pgm.pose(rng.normal(size=3), 0.7, rng.normal(size=3)), pgm.pose(rng.normal(size=3), 1.9, rng.normal(size=3))
    ab = np.array([True])
    err = pgm.edge_error(X[None], X[None], G[None], np.eye(6)[None], ab)
    assert np.allclose(err["D"][0], np.linalg.inv(G) @ X, atol=1e-14)
    _, Jj = pgm.jacobians(err, G[None], ab)
    num = np.zeros((6, 6))
    for c in range(6):
        d = np.zeros(6); d[c] = 1e-6
        p, m = pgm.retract(X, d), pgm.retract(X, -d)
        num[:, c] = (pgm.edge_error(p[None], p[None], G[None], np.eye(6)[None], ab)["e"][0]
                     - pgm.edge_error(m[None], m[None], G[None], np.eye(6)[None], ab)["e"][0]) / 2e-6
    assert np.abs(Jj[0] - num).max() <= 1e-7


def test_circle_problem_dense():
    g, _ = pgc.circle()
    gap0 = np.linalg.norm(g.X[100, :3, 3] - g.X[0, :3, 3])
    r = pgm.optimize(g, iters=20)
    gap = np.linalg.norm(g.X[100, :3, 3] - g.X[0, :3, 3])
    print("chi2 %.6g -> %.6g, gap %.3g -> %.3g m, %d steps" % (r["chi2_0"], r["chi2"], gap0, gap, len(r["steps"])))
    assert r["chi2"] * 100.0 < r["chi2_0"] and gap < 1e-3
    assert np.abs(g.X[:, :3, :3] @ np.swapaxes(g.X[:, :3, :3], 1, 2) - np.eye(3)).max() < 1e-14


@pytest.mark.parametrize("name", ["n1", "n2", "no_loop"])
def test_trivial_chain_comes_back_bit_for_bit(name):
    g = pgc.CASES[name]()
    before = g.X.copy()
    r = pgm.optimize(g)
    assert r["status"] == pgm.CONVERGED | pgm.TRIVIAL and np.array_equal(g.X, before) and r["chi2"] == 0.0
    assert np.all(pgm.chi_terms(g, g.X) <= 1e-25)                    # the chain is satisfied as appended


@pytest.mark.parametrize("name", pgc.OPTIMISED)
def test_conditioning_of_every_case(name):
    g = pgc.CASES[name]()
    slots, table = pgm.linearise(g)
    H, _ = pgm.assemble(g, slots, table)
    cond = pgm.scaled_condition(g, H, 1e-5 * np.max(np.diag(H)[pgm.free_index(g)]))
    print("%s: cond %.3g" % (name, cond))
    assert cond <= 1e6


@pytest.mark.parametrize("name", [k for k in pgc.OPTIMISED if k not in ("n257", "circle")])   # (those two are still moving after 20 iterations)
def test_cg_agrees_with_dense(name):
    a, b = pgc.CASES[name](), pgc.CASES[name]()
    ra, rb = pgm.optimize(a, solver="dense"), pgm.optimize(b, solver="cg")
    dt, dr = pgm.distance(a.X, b.X)
    assert ra["chi2"] < ra["chi2_0"] and dt < 1e-6 and dr < 1e-6 and abs(ra["chi2"] - rb["chi2"]) <= 1e-6 * ra["chi2"]


def test_block_sum_order():
    v = np.random.default_rng(3).normal(size=1000) * 10.0 ** np.random.default_rng(4).integers(-8, 8, 1000)
    assert pgm.block_sum(v) == pgm.block_sum(np.concatenate([v, np.zeros(37)]))
    assert abs(pgm.block_sum(v) - np.sum(v)) <= 1e-12 * np.abs(v).sum()
    assert pgm.block_sum([1.0, 2.0, 3.0]) == 6.0 and pgm.block_sum([]) == 0.0


def test_default_information_rules():
    assert np.array_equal(pgm.default_information("loop", 2, 6), pgm.OM_ODOMETRY)
    assert np.array_equal(pgm.default_information("loop", 2, 7), pgm.OM_LOOP_FAR)
    assert np.array_equal(pgm.default_information("absolute"), np.diag([1, 1, 1, .001, .001, .001]))
    assert np.array_equal(pgc.CASES["rule_at_4"]().loops[0][3], pgm.OM_ODOMETRY)
    assert np.array_equal(pgc.CASES["rule_at_5"]().loops[0][3], pgm.OM_LOOP_FAR)


# ---- planted faults: each must change a table row ---------------------------------------------------------------------------

def test_fault_sign_rule_dropped():
    assert _jacobian_error(("no_sign_rule",))[0] > 1e-2


def test_fault_z_for_z_inverse():
    g = pgc.CASES["one_loop"]()
    good, bad = pgm.chi_terms(g, g.X).sum(), pgm.chi_terms(g, g.X, ("z_for_zinv",)).sum()
    assert bad > 100.0 * good


def test_fault_loop_rule_at_5():
    assert not np.array_equal(pgm.default_information("loop", 2, 7, ("loop_rule_5",)), pgm.default_information("loop", 2, 7))


def test_fault_fixed_row_left_in():
    a, b = pgc.CASES["one_loop"](), pgc.CASES["one_loop"]()
    pgm.optimize(a); pgm.optimize(b, faults=("fixed_row_in",))
    assert np.array_equal(a.X[0], np.eye(4)) and not np.array_equal(b.X[0], np.eye(4))


def test_fault_reject_keeps_trial():
    g = pgc.CASES["one_loop"]()
    slots, _ = pgm.linearise(g)
    b = pgm.gather_b(g, slots)
    H, bb = pgm.assemble(g, slots, pgm.linearise(g)[1])
    delta = 40.0 * pgm.solve(g, H, bb, 1e-3)[0]                     # an overshoot that raises chi2: rejected
    chi = pgm.block_sum(slots[:, pgm.CHI])
    good = pgm.judge(g, g.X, delta, b, 1e-3, 2.0, chi)
    bad = pgm.judge(g, g.X, delta, b, 1e-3, 2.0, chi, ("reject_keeps_trial",))
    assert not good["accepted"] and good["lam"] == 2e-3 and good["nu"] == 4.0
    assert np.array_equal(good["X"], g.X) and not np.array_equal(bad["X"], g.X)
