"""Problems of the robust-kernel tests, shared by the CPU and GPU tests: the scene with one false
loop, and a table of edges whose raw term ``c = e^T Omega e`` is exact.

The table's graph is a chain of three vertices at x = 0, 1, 2 (pure translations, dyadic values).  A loop (0, 2) measured
as a translation of 1 has the error e = (1, 0, 0, 0, 0, 0), so with Omega = diag(c, 1, 1, 1, 1, 1) its raw term is c
exactly, whatever double c is: the knees of the kernels can be met, and missed by one unit in the last place, on purpose.
"""
import numpy as np

import pose_graph_cases as pgc
import pose_graph_model as pgm
from pose_graph_robust_model import Robust

# ---- the scene: five correct loops and one false one over a drifting chain ---------------------------------------------------

SCENE_LOOPS = [(0, 50), (5, 55), (10, 58), (2, 45), (8, 52)]
SCENE_FALSE = (3, 40)
SCENE_OMEGA = np.diag([100.0, 100, 100, 400, 400, 400])
SCENE_ROBUST = Robust("geman_mcclure", 1.0, ("loop",))


def scene(false_loop=True, N=None, noise=(0.005, 0.02), ML=8, MA=8):
    """-> (Graph of 60 vertices, gt).  The false loop, where asked for, is the last loop (index 5)."""
    g, gt = pgc.noisy_chain(60, seed=3, N=N, ML=ML, MA=MA, noise=noise)
    for i, j in SCENE_LOOPS:
        g.add_loop(i, j, pgc.between(gt, i, j), SCENE_OMEGA)
    if false_loop:
        i, j = SCENE_FALSE
        g.add_loop(i, j, pgc.between(gt, i, j) @ pgm.pose([0, 0, 1], 0.3, [3, -2, 0.5]), SCENE_OMEGA)
    return g, gt


# ---- the edge table ----------------------------------------------------------------------------------------------------------

def trans(x, y=0.0, z=0.0):
    T = np.eye(4)
    T[:3, 3] = (x, y, z)
    return T


def omega_c(c):
    om = np.eye(6)
    om[0, 0] = c
    return om


def chain3(N=4, ML=2, MA=2):
    g = pgm.Graph(N, ML, MA, True)
    g.append(trans(1.0))
    g.append(trans(1.0))
    return g


def loop_with(c=None, Z=None, Om=None):
    """The three-vertex chain and the loop (0, 2) with raw term c (or the measurement and information given)."""
    def build():
        g = chain3()
        g.add_loop(0, 2, trans(1.0) if Z is None else Z, omega_c(c) if Om is None else Om)
        return g
    return build


def every_class(om_loop=None, om_abs=None):
    """The chain with its last vertex moved to x = 3, so that every class has an edge with a raw term above the knees used
    with it: chain edge 1 at c = 0, chain edge 2 (e_x = 1, Omega = diag(2,2,2,5,5,5)) at c = 2, the loop (0, 2) measured as 1
    (e_x = 2) at c = 4, an absolute edge on vertex 2 measured at x = 1 (e_x = 2) at c = 4, one on vertex 1 at c = 0."""
    def build():
        g = chain3(MA=3)
        g.X[2] = trans(3.0)
        g.add_loop(0, 2, trans(1.0), np.eye(6) if om_loop is None else om_loop)
        g.add_absolute(2, trans(1.0), np.eye(6) if om_abs is None else om_abs)
        g.add_absolute(1, trans(1.0), np.eye(6))
        return g
    return build


def _neighbours(x):
    return [("below", float(np.nextafter(x, -np.inf))), ("at", float(x)), ("above", float(np.nextafter(x, np.inf)))]


def _table():
    rows = {}
    d0 = 1.5                                       # delta (Phi for DCS): delta^2 = 2.25 is exact
    knee = {"huber": d0 * d0, "geman_mcclure": d0, "dcs": d0}      # (Geman-McClure has no knee: c = delta is where a = 1/2)
    for kernel in ("huber", "geman_mcclure", "dcs"):
        for where, c in _neighbours(knee[kernel]):                 # c at the knee and at both of its neighbours
            rows["%s_c_%s_knee" % (kernel, where)] = (loop_with(c), Robust(kernel, d0))
        for where, d in _neighbours(d0):                           # delta at both of its neighbours, c at the knee of d0
            if where != "at":
                rows["%s_delta_%s" % (kernel, where)] = (loop_with(knee[kernel]), Robust(kernel, d))
        rows[kernel + "_c_0"] = (loop_with(Z=trans(2.0), Om=np.eye(6)), Robust(kernel, d0))
        rows[kernel + "_c_1"] = (loop_with(1.0), Robust(kernel, 0.5))
        rows[kernel + "_c_1e300"] = (loop_with(1e300), Robust(kernel, d0))
        rows[kernel + "_c_not_finite"] = (loop_with(Z=trans(np.inf), Om=np.eye(6)), Robust(kernel, d0))
        for edges in (("chain",), ("loop",), ("absolute",), ("chain", "loop", "absolute")):
            rows["%s_on_%s" % (kernel, "_".join(edges))] = (every_class(), Robust(kernel, 0.5, edges))
        rows[kernel + "_full_omega"] = (every_class(pgc.full_omega(31), pgc.full_omega(32)),
                                        Robust(kernel, 0.5, ("loop", "absolute")))
    return rows


TABLE = _table()
