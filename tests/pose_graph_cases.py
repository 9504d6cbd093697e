"""Table of pose-graph problems shared by the CPU and GPU tests: small noisy chains with every edge
placement the kernels treat differently, and the reference's circle problem."""
import numpy as np

import pose_graph_model as pgm


def noisy_chain(n, seed, N=None, ML=8, MA=8, fix_first=True, noise=(0.02, 0.05)):
    """-> (Graph of n vertices, gt (n, 4, 4)): about 1 m forward per step with a gentle turn; the chain measurements carry noise
    (rad, m), so exact long-range measurements disagree with it."""
    rng = np.random.default_rng(seed)
    g = pgm.Graph(n if N is None else N, ML, MA, fix_first)
    gt = [np.eye(4)]
    for _ in range(1, n):
        step = pgm.pose(rng.normal(size=3) + [0, 0, 3.0], rng.normal(0.0, 0.08), [1.0 + rng.normal(0, 0.1), rng.normal(0, 0.1), rng.normal(0, 0.02)])
        gt.append(gt[-1] @ step)
        g.append(step @ pgm.pose(rng.normal(size=3), rng.normal(0.0, noise[0]), rng.normal(0.0, noise[1], 3)))
    return g, np.array(gt)


def between(gt, i, j):
    return np.linalg.inv(gt[i]) @ gt[j]


def full_omega(seed):
    a = np.random.default_rng(seed).normal(size=(6, 6))
    om = a @ a.T + 6.0 * np.eye(6)
    return (om + om.T) / 2.0


def circle(N=None, seed=0):
    """The reference's problem (its tests/test_backend.py): 101 poses at the angles 2 pi k / 101 of a circle of radius 10, every
    relative pose multiplied by a noise transform of 0.1 rad (three Euler angles, N(0, 0.1) each) and 0.1 m (N(0, 0.1) per
    axis) from a fixed seed, one loop (0, 100) at Z = I with Omega = 1e6 I."""
    rng = np.random.default_rng(seed)
    n = 101
    th = 2.0 * np.pi * np.arange(n) / n
    gt = np.array([pgm.pose([0, 0, 1], -t, [10 * np.cos(t), -10 * np.sin(t), 0.0]) for t in th])
    gt = np.linalg.inv(gt[0])[None] @ gt
    g = pgm.Graph(n if N is None else N, 8, 8, True)
    for k in range(1, n):
        a, t = rng.normal(0.0, 0.1, 3), rng.normal(0.0, 0.1, 3)
        noise = pgm.pose([0, 0, 1], a[2]) @ pgm.pose([0, 1, 0], a[1]) @ pgm.pose([1, 0, 0], a[0], t)
        g.append(between(gt, k - 1, k) @ noise)
    g.add_loop(0, n - 1, np.eye(4), 1e6 * np.eye(6))
    return g, gt


def _one(n, seed, **kw):
    g, gt = noisy_chain(n, seed, **kw)
    if n >= 3:
        g.add_loop(0, n - 1, between(gt, 0, n - 1))
    return g


def _placed(n, seed, loops=(), absolutes=(), omega=None, **kw):
    g, gt = noisy_chain(n, seed, **kw)
    for i, j in loops:
        g.add_loop(i, j, between(gt, i, j), omega)
    for i in absolutes:
        g.add_absolute(i, gt[i], omega)
    return g


CASES = {
    "n1": lambda: _one(1, 1), "n2": lambda: _one(2, 2), "n3": lambda: _one(3, 3), "n63": lambda: _one(63, 4),
    "n64": lambda: _one(64, 5), "n65": lambda: _one(65, 6), "n257": lambda: _one(257, 7),
    "no_loop": lambda: _placed(9, 8),
    "one_loop": lambda: _placed(12, 9, [(2, 10)]),
    "three_share_a_vertex": lambda: _placed(14, 10, [(1, 7), (1, 9), (1, 12)]),
    "first_and_last": lambda: _placed(13, 11, [(0, 6), (5, 12)]),
    "absolute_on_0_free": lambda: _placed(10, 12, [(1, 8)], [0], fix_first=False),
    "absolute_and_loop": lambda: _placed(10, 13, [(0, 9)], [4, 9]),
    "rule_at_4": lambda: _placed(10, 14, [(2, 6)]),
    "rule_at_5": lambda: _placed(10, 14, [(2, 7)]),
    "full_omega": lambda: _placed(11, 15, [(1, 9)], [5], omega=full_omega(15)),
    "circle": lambda: circle()[0],
}
OPTIMISED = [k for k in CASES if k not in ("n1", "n2", "no_loop")]     # the cases with something to optimise
