"""CPU tests of the robust-kernel model and its tables: the weights against central differences,
continuity at the knees, the scene with one false loop, a second implementation written edge by edge as the kernel is, the
planted faults (each must change a table row), the host's refusals and the facade's property."""
import numpy as np
import pytest

import pose_graph_model as pgm
import pose_graph_robust_cases as prc
import pose_graph_robust_model as prm

KERNELS = ("huber", "geman_mcclure", "dcs")
FAULTS = ("w_on_gradient_only", "w_on_blocks_only", "chi_only_keeps_c", "huber_delta_for_delta2", "mask_off_by_one")


def same(a, b):
    """Equal to the bit where a number is meant; a NaN matches a NaN (its sign and payload are the processor's)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


# ---- rho and w ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("delta", [0.5, 1.0, 3.0])
def test_weight_is_the_derivative_of_rho(kernel, delta):
    """Central differences at step h = 1e-6 max(1, c): truncation h^2 |rho'''| / 6 <= 1e-11 and rounding 2^-52 rho / h <=
    1e-8 for rho <= 50, so 1e-7 holds both; c within 1e-3 of a knee is left out (w jumps in slope there).

    DCS past its knee is left out as well, and shown to differ: there the specification (as g2o's DCS does) scales the edge by
    w = s^2 and reports rho = s^2 c, which is the scaled term, not an antiderivative of w; inside the knee rho = c, w = 1."""
    kind, knee = prm.KINDS[kernel], {"huber": delta * delta, "geman_mcclure": None, "dcs": delta}[kernel]
    worst = 0.0
    for c in (0.1, 0.2, 0.7, 1.3, 3.0, 8.0, 10.0, 50.0):
        h = 1e-6 * max(1.0, c)
        if knee is not None and abs(c - knee) <= 1e-3:
            continue
        (lo, hi), w = prm.rho_w(kind, delta, np.array([c - h, c + h]))[0], float(prm.rho_w(kind, delta, c)[1])
        if kernel == "dcs" and c > knee:
            assert abs((hi - lo) / (2 * h) - w) > 1e-4
            continue
        worst = max(worst, abs((hi - lo) / (2 * h) - w))
    print("%s delta %g: max |central difference - w| = %.3g" % (kernel, delta, worst))
    assert worst <= 1e-7


@pytest.mark.parametrize("kernel,knee_of", [("huber", lambda d: d * d), ("dcs", lambda d: d)])
@pytest.mark.parametrize("delta", [0.5, 1.0, 1.5, 3.0])
def test_rho_and_w_are_continuous_at_the_knee(kernel, knee_of, delta):
    """Across the knee's two fp64 neighbours rho moves by a few units in its last place (rho' <= 1) and w leaves 1 by as
    little."""
    knee = knee_of(delta)
    c = np.array([np.nextafter(knee, -np.inf), knee, np.nextafter(knee, np.inf)])
    rho, w = prm.rho_w(prm.KINDS[kernel], delta, c)
    eps = np.finfo(np.float64).eps
    assert rho[0] == c[0] and rho[1] == c[1] and w[0] == 1.0 and w[1] == 1.0          # the knee itself is inside
    assert abs(rho[2] - rho[1]) <= 8 * eps * knee and abs(w[2] - 1.0) <= 8 * eps
    assert np.all(np.diff(rho) >= -8 * eps * knee)


@pytest.mark.parametrize("kernel", KERNELS)
def test_non_finite_c_gives_non_finite_rho(kernel):
    rho, w = prm.rho_w(prm.KINDS[kernel], 1.5, np.array([np.inf, np.nan, 1e300, 0.0]))
    assert not np.isfinite(rho[0]) and not np.isfinite(rho[1]) and np.isfinite(rho[2]) and rho[3] == 0.0 and w[3] == 1.0
    assert 0.0 <= w[2] < 1e-100


# ---- the scene -----------------------------------------------------------------------------------------------------------------

def _scene_run(rb, false_loop=True, noise=(0.005, 0.02)):
    g, _ = prc.scene(false_loop, noise=noise)
    start = g.X.copy()
    r = prm.optimize(g, rb, iters=30)
    return g, r, start


@pytest.mark.parametrize("noise", [(0.005, 0.02), (0.02, 0.05)])
def test_scene_geman_mcclure_rejects_the_false_loop(noise):
    """Conditions on the scene, not tolerances on any implementation: with Geman-McClure, delta = 1, on the loops every
    correct loop keeps w >= 0.9, the false loop ends at w <= 0.1, and the result lies closer to the clean graph's than
    without a kernel."""
    clean, _, _ = _scene_run(None, false_loop=False, noise=noise)
    plain, _, _ = _scene_run(None, noise=noise)
    robust, r, _ = _scene_run(prc.SCENE_ROBUST, noise=noise)
    w = prm.edge_weights(robust, prc.SCENE_ROBUST)[:6, 1]
    d_plain, d_robust = pgm.distance(clean.X, plain.X), pgm.distance(clean.X, robust.X)
    print("to clean: no kernel %.3g m %.3g rad, Geman-McClure %.3g m %.3g rad (status %d); weights %s"
          % (d_plain + d_robust + (r["status"], np.round(w, 4).tolist())))
    assert np.all(w[:5] >= 0.9) and w[5] <= 0.1
    assert d_robust[0] < d_plain[0] and d_robust[1] < d_plain[1]


def test_scene_dcs_and_huber_findings():
    """Properties of the kernels on this scene (section 25.1), recorded so that nobody takes them for bugs: DCS with Phi = 1
    switches the correct loops off as well (the drift makes every loop's first chi2 far larger than Phi), and Huber never
    engages (the weak odometry lets the graph bend until the false loop's chi2 is below delta^2)."""
    dcs = prm.Robust("dcs", 1.0)
    g, _, start = _scene_run(dcs)
    w = prm.edge_weights(g, dcs)[:6, 1]
    assert np.all(w <= 0.1) and pgm.distance(start, g.X)[0] <= 0.5
    plain, _, _ = _scene_run(None)
    for delta in (1.0, 3.0):
        hub = prm.Robust("huber", delta)
        g, _, _ = _scene_run(hub)
        assert np.all(prm.edge_weights(g, hub)[:6, 1] == 1.0) and max(pgm.distance(plain.X, g.X)) <= 1e-2


# ---- a second implementation, edge by edge as the kernel runs ------------------------------------------------------------------

def _robustify(kind, delta, c, faults=()):
    """pg_robustify for one edge, with numpy scalars so that inf and nan pass through silently."""
    c, delta = np.float64(c), np.float64(delta)
    with np.errstate(all="ignore"):
        if kind == 1:
            knee = delta if "huber_delta_for_delta2" in faults else delta * delta
            if (c < knee) if "knee_lt" in faults else (c <= knee):
                return c, np.float64(1.0)
            s = np.sqrt(c)
            return (2.0 * s) * delta - delta * delta, delta / s
        if kind == 2:
            a = delta / (delta + c)
            return c * a, a * a
        if kind == 3:
            s = (2.0 * delta) / (delta + c)
            if (s > 1.0) if "knee_lt" in faults else (s >= 1.0):
                return c, np.float64(1.0)
            w = s * s
            return w * c, w
    return c, np.float64(1.0)


def kernel_form(g, rb, X=None, full=True, faults=()):
    """What one launch leaves: full -> slots (E, 136), otherwise the chi2 terms (E,).  One edge at a time: its class from its
    id, rho and w, then the finished blocks and gradients of the plain linearisation times w."""
    X = g.X if X is None else X
    plain, (ids, vi, vj, ab) = pgm.linearise(g, X)
    slots, chi = np.zeros_like(plain), np.zeros(g.E)
    for k, id_ in enumerate(ids):
        cls = 1 if id_ < g.N else 2 if id_ < g.N + g.ML else 4
        if "mask_off_by_one" in faults:
            cls = {1: 2, 2: 4, 4: 1}[cls]
        c = plain[id_, pgm.CHI]
        rho, w = _robustify(rb.kind if rb.mask & cls else 0, rb.delta, c, faults)
        chi[id_] = c if "chi_only_keeps_c" in faults else rho
        sl = plain[id_].copy()
        wb = np.float64(1.0) if "w_on_gradient_only" in faults else w
        wg = np.float64(1.0) if "w_on_blocks_only" in faults else w
        with np.errstate(all="ignore"):
            for lo, hi, f in ((pgm.HJJ, pgm.BI, wb), (pgm.BJ, pgm.CHI, wg)) + \
                    (() if ab[k] else ((pgm.HII, pgm.HJJ, wb), (pgm.BI, pgm.BJ, wg))):
                for m in range(lo, hi):
                    sl[m] = f * sl[m]
        sl[pgm.CHI], sl[prm.RAW], sl[prm.W] = rho, c, w
        slots[id_] = sl
    return slots if full else chi


def _differs(name, faults):
    build, rb = prc.TABLE[name]
    g = build()
    with np.errstate(invalid="ignore"):                                # (the row with the infinite measurement)
        return not (same(kernel_form(g, rb, faults=faults), prm.linearise(g, rb)[0])
                    and same(kernel_form(g, rb, full=False, faults=faults), prm.chi_terms(g, rb, g.X)))


@pytest.mark.parametrize("name", list(prc.TABLE))
def test_second_implementation_equals_the_model(name):
    assert not _differs(name, ())


@pytest.mark.parametrize("name", list(prc.TABLE))
def test_table_rows_are_what_they_say(name):
    """The loop's raw term is the c its row names, exactly; the chi-only pass carries rho, the slot both rho and c."""
    build, rb = prc.TABLE[name]
    g = build()
    with np.errstate(invalid="ignore"):
        slots, (ids, _, _, _) = prm.linearise(g, rb)
        chi_only = prm.chi_terms(g, rb, g.X)
    loop = slots[g.N]
    rho, w = prm.rho_w(rb.kind, rb.delta, loop[prm.RAW])
    if rb.mask & 2:
        assert same(loop[pgm.CHI], rho) and same(loop[prm.W], w)
    else:
        assert loop[pgm.CHI] == loop[prm.RAW] and loop[prm.W] == 1.0
    assert same(chi_only[ids], slots[ids, pgm.CHI])
    kernel = rb.kernel
    knee = 2.25 if kernel == "huber" else 1.5
    expect = {"_c_at_knee": knee, "_c_below_knee": np.nextafter(knee, -np.inf), "_c_above_knee": np.nextafter(knee, np.inf),
              "_delta_below": knee, "_delta_above": knee, "_c_0": 0.0, "_c_1": 1.0, "_c_1e300": 1e300}
    for suffix, c in expect.items():
        if name == kernel + suffix:
            assert loop[prm.RAW] == c
    if name.endswith("_c_not_finite"):
        assert not np.isfinite(loop[prm.RAW]) and not np.isfinite(loop[pgm.CHI])
    if "_on_" in name or name.endswith("_full_omega"):
        w_all = slots[ids, prm.W]
        chosen = (prm.edge_class(g, ids) & rb.mask) != 0
        assert np.all(w_all[~chosen] == 1.0) and np.any(w_all[chosen] < 1.0) and np.all(slots[ids, prm.RAW][chosen] >= 0.0)
    if name.endswith("_c_at_knee") and kernel != "geman_mcclure":
        assert loop[prm.W] == 1.0 and loop[pgm.CHI] == knee
    if name == "huber_c_above_knee":
        assert loop[pgm.CHI] != loop[prm.RAW]                             # one unit past the knee already takes the outer branch


@pytest.mark.parametrize("fault", FAULTS)
def test_every_planted_fault_changes_a_row(fault):
    changed = [name for name in prc.TABLE if _differs(name, (fault,))]
    print("%s changes %d of %d rows, e.g. %s" % (fault, len(changed), len(prc.TABLE), changed[:3]))
    assert changed


def test_strictness_at_a_knee_cannot_show():
    """The planted fault "< for <= at a knee" changes no bit of any row, and cannot: at c = delta^2 Huber's outer branch has
    s = sqrt(c) = delta exactly (the square root of a rounded square is the number itself), so rho = 2 c - c = c and w =
    delta / delta = 1; at c = Phi DCS has s = 1, so w = 1 and rho = c.  Both branches give the inner branch's bits, which is the
    continuity the kernels are built for; the table still holds the knee rows, so a knee moved by one unit would show."""
    for name in prc.TABLE:
        assert not _differs(name, ("knee_lt",)), name
    for delta in (0.1, 0.3, 1.5, 2.0 / 3.0, 1e-3, 7.7e5):
        c = np.float64(delta) * np.float64(delta)
        assert same(_robustify(1, delta, c, ("knee_lt",)), (c, 1.0)) and same(_robustify(3, delta, delta, ("knee_lt",)), (delta, 1.0))


# ---- the host --------------------------------------------------------------------------------------------------------------------

BAD = [dict(kernel="cauchy"), dict(kernel=2), dict(delta=1.0), dict(kernel="huber", delta=0.0), dict(kernel="huber", delta=-1.0),
       dict(kernel="dcs", delta=float("inf")), dict(kernel="dcs", delta=float("nan")), dict(kernel="huber", delta="1"),
       dict(kernel="huber", delta=True), dict(kernel="huber", edges=()), dict(kernel="huber", edges=("loops",)),
       dict(kernel="huber", edges=("loop", "loop")), dict(kernel="huber", sigma=1.0), "huber", ("huber", 1.0)]


@pytest.mark.parametrize("robust", BAD, ids=[str(k) for k in range(len(BAD))])
def test_host_refuses_bad_settings_before_any_launch(robust):
    from pwclonet_pylidarslam_amd import pose_graph
    from pwclonet_pylidarslam_amd.odometry import StreamingOdometry
    with pytest.raises(ValueError, match="robust"):
        pose_graph.robust_settings(robust)
    with pytest.raises(ValueError, match="robust"):
        pose_graph.PoseGraph(1, max_poses=4, robust=robust)              # refused before the library or the device is touched
    with pytest.raises(ValueError, match="robust"):
        StreamingOdometry(object(), backend=dict(source="network", robust=robust))


def test_host_settings_as_the_launches_take_them():
    from pwclonet_pylidarslam_amd.pose_graph import robust_settings
    assert robust_settings(None) is None
    assert robust_settings(dict(kernel="geman_mcclure")) == (2, 1.0, 2)                      # the default: loops only
    assert robust_settings(dict(kernel="huber", delta=3, edges="absolute")) == (1, 3.0, 4)
    assert robust_settings(dict(kernel="dcs", delta=0.25, edges=("absolute", "chain", "loop"))) == (3, 0.25, 7)
    for name, rb in ((n, r) for n, (_, r) in prc.TABLE.items()):
        assert robust_settings(rb.settings()) == (rb.kind, rb.delta, rb.mask), name


def test_graph_slam_robust_kernel_property():
    from pwclonet_pylidarslam_amd.backend import GraphSLAM, RobustKernel
    slam = GraphSLAM()
    assert slam.robust_kernel is None
    k = RobustKernel("geman_mcclure", 2.0)
    slam.robust_kernel = k
    assert slam.robust_kernel is k and slam._robust_settings() == dict(kernel="geman_mcclure", delta=2.0,
                                                                        edges=("chain", "loop", "absolute"))
    assert RobustKernel("huber").delta == 1.0
    slam.robust_kernel = None
    assert slam.robust_kernel is None and slam._robust_settings() is None
    for bad in ("huber", RobustKernel("cauchy"), RobustKernel("huber", 0.0)):
        with pytest.raises(ValueError):
            slam.robust_kernel = bad
        assert slam.robust_kernel is None
