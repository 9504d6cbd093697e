"""Float64 NumPy model of the robust kernels on the pose graph, over pose_graph_model.

For an edge with the raw term ``c = e^T Omega e`` a kernel gives ``rho(c)`` and the weight ``w = rho'(c)``; the edge then brings
``rho`` as its chi2 term and ``w`` times its finished blocks and gradients (first order: no rho'' term).  Every expression is
written in the order of ``pg_robustify`` (csrc/pose_graph.hpp), so the device's chi2 terms, ``c`` and ``w`` agree to the bit.
``linearise``, ``chi_terms`` and ``optimize`` are pose_graph_model's with the kernel applied.
"""
import contextlib

import numpy as np

import pose_graph_model as pgm

RAW, W = 133, 134                                 # csrc/pose_graph.hpp: PG_RAW, PG_W
KINDS = {"huber": 1, "geman_mcclure": 2, "dcs": 3}
CLASSES = {"chain": 1, "loop": 2, "absolute": 4}
_plain_linearise, _plain_chi_terms = pgm.linearise, pgm.chi_terms      # (optimize below swaps the module's names for a call)


class Robust:
    """One kind and one delta per graph, on the edge classes of ``edges``."""

    def __init__(self, kernel, delta=1.0, edges=("loop",)):
        self.kernel, self.delta, self.edges = kernel, float(delta), tuple(edges)
        self.kind = KINDS[kernel]
        self.mask = sum(CLASSES[e] for e in self.edges)

    def settings(self):
        """As ``PoseGraph(robust=...)`` takes it."""
        return dict(kernel=self.kernel, delta=self.delta, edges=self.edges)


def rho_w(kind, delta, c):
    """rho and w at c (any shape), each expression in the kernel's order."""
    c = np.asarray(c, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        if kind == KINDS["huber"]:
            s = np.sqrt(c)
            inside = c <= delta * delta
            return np.where(inside, c, (2.0 * s) * delta - delta * delta), np.where(inside, 1.0, delta / s)
        if kind == KINDS["geman_mcclure"]:
            a = delta / (delta + c)
            return c * a, a * a
        if kind == KINDS["dcs"]:
            s = (2.0 * delta) / (delta + c)
            inside = s >= 1.0
            w = np.where(inside, 1.0, s * s)
            return np.where(inside, c, w * c), w
    return c.copy(), np.ones_like(c)


def edge_class(g, ids):
    """The class bit of every edge id."""
    ids = np.asarray(ids, int)
    return np.where(ids < g.N, CLASSES["chain"], np.where(ids < g.N + g.ML, CLASSES["loop"], CLASSES["absolute"]))


def edge_rho_w(g, rb, ids, c):
    """rho and w of the edges ids with raw terms c: an edge outside the mask keeps rho = c, w = 1."""
    c = np.asarray(c, np.float64)
    if rb is None:
        return c.copy(), np.ones_like(c)
    rho, w = rho_w(rb.kind, rb.delta, c)
    chosen = (edge_class(g, ids) & rb.mask) != 0
    return np.where(chosen, rho, c), np.where(chosen, w, 1.0)


def chi_terms(g, rb, X, faults=()):
    """rho of every edge at the poses X, placed at its id."""
    out = _plain_chi_terms(g, X, faults)
    ids = g.edges()[0]
    if len(ids):
        out[ids] = edge_rho_w(g, rb, ids, out[ids])[0]
    return out


def linearise(g, rb, X=None, faults=()):
    """-> slots (E, 136) and the edge table: pose_graph_model's slots with rho at CHI, every finished block and gradient
    times w, and (c, w) in the doubles 133 and 134.  The i side of an absolute edge, which no kernel writes, stays zero."""
    slots, table = _plain_linearise(g, X, faults)
    ids, _, _, ab = table
    if rb is None or not len(ids):
        return slots, table
    s = slots[ids]
    c = s[:, pgm.CHI].copy()
    rho, w = edge_rho_w(g, rb, ids, c)
    with np.errstate(invalid="ignore", over="ignore"):
        s[:, pgm.HII:pgm.CHI] = w[:, None] * s[:, pgm.HII:pgm.CHI]
    for lo, hi in ((pgm.HII, pgm.HJJ), (pgm.BI, pgm.BJ)):
        s[np.ix_(ab, range(lo, hi))] = 0.0
    s[:, pgm.CHI], s[:, RAW], s[:, W] = rho, c, w
    slots[ids] = s
    return slots, table


def edge_weights(g, rb, X=None):
    """(ML + MA, 2): (c, w) of the loops and the absolute edges at X, zeros past the edges in use."""
    X = g.X if X is None else X
    out = np.zeros((g.ML + g.MA, 2))
    ids = g.edges()[0]
    if len(ids):
        c = _plain_chi_terms(g, X)[ids]
        w = edge_rho_w(g, rb, ids, c)[1]
        long = ids >= g.N
        out[ids[long] - g.N] = np.stack([c[long], w[long]], -1)
    return out


@contextlib.contextmanager
def _applied(rb):
    """pose_graph_model.optimize and .judge reach linearise and chi_terms by name: for the time of one call they are the
    robust ones."""
    pgm.linearise = lambda g, X=None, faults=(): linearise(g, rb, X, faults)
    pgm.chi_terms = lambda g, X, faults=(): chi_terms(g, rb, X, faults)
    try:
        yield
    finally:
        pgm.linearise, pgm.chi_terms = _plain_linearise, _plain_chi_terms


def optimize(g, rb, iters=20, solver="dense", pcg_tol=1e-8, pcg_iters=None, faults=()):
    """pose_graph_model.optimize on the robustified graph: LM, lambda_0, the gain ratio, the convergence rule and the status
    bits are its own and see rho in place of c."""
    if rb is None:
        return pgm.optimize(g, iters, solver, pcg_tol, pcg_iters, faults)
    with _applied(rb):
        return pgm.optimize(g, iters, solver, pcg_tol, pcg_iters, faults)
