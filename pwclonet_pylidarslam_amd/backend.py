"""The reference's ``slam.backend`` interface over the device pose graph.

``GraphSLAM`` keeps one stream of ``pose_graph.PoseGraph`` and speaks the reference's protocol: NumPy in and out, the
constraints of a frame found in its ``data_dict`` under the keys the static builders below make.  There is no g2o and no CPU
path: the optimisation runs on the device.
"""
import re
from dataclasses import dataclass

import numpy as np
import torch

from .pose_graph import EDGE_CLASSES, PoseGraph, default_information, robust_settings


def _mul(a, b):
    """a . b of two rigid transforms in the order of the device's product, so that a chain rebuilt here has the bits of one
    appended there."""
    c = np.eye(4)
    for i in range(3):
        for j in range(4):
            s = (a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j]
            c[i, j] = s + a[i, 3] if j == 3 else s
    return c


@dataclass(frozen=True)
class RobustKernel:
    """What ``GraphSLAM.robust_kernel`` takes in place of a g2o kernel object: ``name`` "huber", "geman_mcclure" or "dcs"
    and its ``delta`` (g2o's ``setDelta``; Phi for "dcs")."""
    name: str
    delta: float = 1.0

    def settings(self):
        """As ``PoseGraph(robust=...)`` takes it, on all three edge classes: the reference sets the kernel on every edge."""
        return dict(kernel=self.name, delta=self.delta, edges=tuple(EDGE_CLASSES))


@dataclass
class GraphSLAMConfig:
    initialize_world_coordinates: bool = True
    fix_first_frame: bool = True
    max_optim_iterations: int = 100
    online_optimization: bool = True
    max_poses: int = 4096
    max_loops: int = 256
    max_absolute: int = 256
    device: str = "cuda"


class GraphSLAM:
    """``next_frame(data_dict)`` reads ``se3_odometry_constraint_<i>`` (the pose of frame i + 1 in frame i),
    ``se3_loop_closure_constraint_<i>_<j>`` (the pose of j in i) and ``se3_absolute_constraint_<i>``, each a tuple (4 x 4
    matrix, 6 x 6 information or None), and optimises when it added a loop or an absolute edge.  Odometry constraints must
    arrive in order, one per new frame, with information None or the default's: the chain's is fixed on the device, and any
    other matrix is refused with ValueError, not dropped."""

    def __init__(self, config=None, **kwargs):
        self.config = config if config is not None else GraphSLAMConfig(**kwargs)
        self._constraints = None
        self.need_to_update_pose = False
        self._graph = None
        self._robust_kernel = None

    @property
    def robust_kernel(self):
        """None or a ``RobustKernel``.  *Departure:* the reference hands the kernel to the edges ``next_frame`` adds after
        the assignment; here it acts on every chain, loop and absolute edge of the graph from the next ``optimize`` on."""
        return self._robust_kernel

    @robust_kernel.setter
    def robust_kernel(self, robust_kernel):
        if robust_kernel is not None:
            if not isinstance(robust_kernel, RobustKernel):
                raise ValueError("GraphSLAM: robust_kernel must be None or a RobustKernel(name, delta), not %r"
                                 % (robust_kernel,))
            robust_settings(robust_kernel.settings(), "GraphSLAM.robust_kernel")
        self._robust_kernel = robust_kernel
        if self._graph is not None:
            self._graph.set_robust(self._robust_settings())

    def _robust_settings(self):
        return None if self._robust_kernel is None else self._robust_kernel.settings()

    @staticmethod
    def _regexes():
        return "^se3_odometry_constraint_([\\d]+)$", "^se3_loop_closure_constraint_([\\d]+)_([\\d]+)$", \
               "^se3_absolute_constraint_([\\d]+)$"

    @staticmethod
    def se3_odometry_constraint(reference_idx):
        return "se3_odometry_constraint_%d" % int(reference_idx)

    @staticmethod
    def se3_loop_closure_constraint(reference_idx, tgt_idx):
        return "se3_loop_closure_constraint_%d_%d" % (int(reference_idx), int(tgt_idx))

    @staticmethod
    def se3_absolute_constraint(reference_idx):
        return "se3_absolute_constraint_%d" % int(reference_idx)

    def need_to_synchronise_poses(self):
        if self.need_to_update_pose:
            self.need_to_update_pose = False
            return True
        return False

    def init(self):
        self.clear()
        self._constraints = {"se3_odometry": [], "se3_loop_closure": [], "se3_absolute": []}

    def clear(self):
        c = self.config
        if self._graph is None:
            self._graph = PoseGraph(1, c.max_poses, c.max_loops, c.max_absolute, iters=c.max_optim_iterations,
                                    fix_first=c.fix_first_frame, device=c.device, robust=self._robust_settings())
        else:
            self._graph.reset()
        self._constraints = None
        self.need_to_update_pose = False

    def pose_graph(self):
        """The ``PoseGraph`` behind the facade."""
        return self._graph

    def _registered(self, kind):
        return [] if self._constraints is None else self._constraints[kind]

    def registered_loop_constraints(self):
        return self._registered("se3_loop_closure")

    def registered_odometry_constraints(self):
        return self._registered("se3_odometry")

    def registered_absolute_constraints(self):
        return self._registered("se3_absolute")

    def search_constraints(self, data_dict):
        found = {"se3_odometry": [], "se3_loop_closure": [], "se3_absolute": []}
        reg_odom, reg_loop, reg_abs = self._regexes()
        for key, value in data_dict.items():
            for kind, reg in (("se3_odometry", reg_odom), ("se3_loop_closure", reg_loop), ("se3_absolute", reg_abs)):
                m = re.search(reg, key) if isinstance(key, str) else None
                if m is not None:
                    matrix, information = value
                    if not isinstance(matrix, np.ndarray):
                        raise ValueError("GraphSLAM: the constraint %s must hold a numpy matrix" % key)
                    found[kind].append(tuple(int(v) for v in m.groups()) + (matrix, information))
        found["se3_odometry"].sort(key=lambda c: c[0])
        for kind in found:
            self._constraints[kind] += found[kind]
        return found

    def next_frame(self, data_dict):
        if self._constraints is None:
            raise RuntimeError("GraphSLAM: init() comes before the first frame")
        g = self._graph
        found = self.search_constraints(data_dict)
        for i, matrix, information in found["se3_odometry"]:
            if information is not None and not np.array_equal(np.asarray(information), default_information("odometry")):
                raise ValueError("GraphSLAM: odometry constraint %d carries an information matrix of its own; the chain's is "
                                 "diag(2,2,2,5,5,5) on the device (pass None)" % i)
            n = int(g.counts()[0])
            if i != n - 1:
                raise ValueError("GraphSLAM: odometry constraint %d out of order (the graph holds %d poses)" % (i, n))
            g.append(torch.from_numpy(np.ascontiguousarray(matrix, dtype=np.float64)).to(g.device)[None])
            if g.overflowed():
                raise RuntimeError("GraphSLAM: more than max_poses=%d poses" % self.config.max_poses)
        for i, j, matrix, information in found["se3_loop_closure"]:
            g.add_loop(0, min(i, j), max(i, j), matrix if i < j else np.linalg.inv(matrix), information)
        for i, matrix, information in found["se3_absolute"]:
            g.add_absolute(0, i, matrix, information)
        if found["se3_loop_closure"] or found["se3_absolute"]:
            if not self.config.online_optimization:                       # start again from the odometry
                rel = g.relative_poses(0).cpu().numpy()
                X = np.empty_like(rel)
                X[0] = np.eye(4)
                for k in range(1, len(rel)):
                    X[k] = _mul(X[k - 1], rel[k])
                g.poses(0).copy_(torch.from_numpy(X))
            self.optimize(self.config.max_optim_iterations)
            self.need_to_update_pose = True

    def optimize(self, max_num_epochs=20):
        self._graph.optimize(min(int(max_num_epochs), self._graph.iters))

    def absolute_poses(self):
        """(n, 4, 4): the poses in the first pose's frame."""
        X = self._graph.poses(0).cpu().numpy()
        return np.linalg.inv(X[0])[None] @ X

    def world_poses(self):
        """(n, 4, 4): the vertices as optimised (they differ from ``absolute_poses`` once absolute constraints move vertex
        0)."""
        return self._graph.poses(0).cpu().numpy().copy()

    def relative_odometry_poses(self):
        """(n, 4, 4): row 0 the identity, row k the pose of frame k in frame k - 1 after optimisation."""
        X = self._graph.poses(0).cpu().numpy()
        out = np.tile(np.eye(4), (len(X), 1, 1))
        out[1:] = np.linalg.inv(X[:-1]) @ X[1:]
        return out
