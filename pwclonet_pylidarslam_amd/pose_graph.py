"""Pose-graph backend on the device: SE(3) graph optimisation per stream.

The reference's ``slam/backend.py`` (``GraphSLAM`` over g2o) as HIP kernels in fp64: per stream a graph of odometry, loop
and absolute constraints, optimised by Levenberg-Marquardt with g2o's schedule; the linear systems are solved by block-Jacobi
preconditioned conjugate gradients, one workgroup per stream.

    pg = PoseGraph(streams=S, max_poses=4096)
    pg.append(rel)                           # (S, 4, 4) fp64 or (S, 7) fp32 rows on the device, once per frame
    pg.add_loop(0, 14, 3120, T)              # host integers: "frame 3120 of stream 0 is frame 14 again", T = pose of j in i
    pg.optimize()
    pg.poses(stream=0)                       # (count, 4, 4) fp64 device view

The kernels are ``csrc/pose_graph.hip``.  There is no CPU path.
"""
import numpy as np
import torch

from . import _lib
from .stream_engine import need as _need, ptr as _p
from .stream_engine import Replay, Replayed, need_iters, stream_count, stream_index, stream_indices

MAX_STREAMS = 1024                               # csrc/pose_graph.hpp
SLOT = 136
WORK_PER_VERTEX = 66
CONVERGED, TRIVIAL, NONFINITE = 1, 2, 4          # status bits (an idle stream keeps its word)
OM_ODOMETRY = (2.0, 2.0, 2.0, 5.0, 5.0, 5.0)     # slam/backend.py:348-358, as diagonals
OM_LOOP_FAR = (0.1, 0.1, 0.1, 0.5, 0.5, 0.5)
OM_ABSOLUTE = (1.0, 1.0, 1.0, 0.001, 0.001, 0.001)
NEAR = 4                                         # loops with |i - j| <= 4 get the odometry information
SLOT_RAW, SLOT_W = 133, 134                      # the robust linearise's raw e^T Omega e and weight (csrc/pose_graph.hpp)
ROBUST_KERNELS = {"huber": 1, "geman_mcclure": 2, "dcs": 3}
EDGE_CLASSES = {"chain": 1, "loop": 2, "absolute": 4}


def default_information(kind, i=0, j=0):
    """The information matrix an edge gets where the caller gives none: kind "odometry", "loop" or "absolute"."""
    if kind == "absolute":
        return np.diag(OM_ABSOLUTE)
    return np.diag(OM_ODOMETRY if kind == "odometry" or abs(int(i) - int(j)) <= NEAR else OM_LOOP_FAR)


def robust_settings(robust, what="PoseGraph"):
    """``robust=`` checked and as the launches take it: None, or (kind, delta, edge mask) from ``dict(kernel="huber" |
    "geman_mcclure" | "dcs", delta=1.0, edges=("loop",))``.  Anything else is refused with ValueError."""
    if robust is None:
        return None
    if not isinstance(robust, dict):
        raise ValueError("%s: robust=%r must be None or a dict(kernel=, delta=, edges=)" % (what, robust))
    unknown = set(robust) - {"kernel", "delta", "edges"}
    if unknown or "kernel" not in robust:
        raise ValueError("%s: robust=dict(...) takes kernel (required), delta and edges, not %s" % (what, sorted(unknown)))
    name = robust["kernel"]
    if not isinstance(name, str) or name not in ROBUST_KERNELS:
        raise ValueError("%s: robust=dict(kernel=%r): one of %s" % (what, name, sorted(ROBUST_KERNELS)))
    delta = robust.get("delta", 1.0)
    if isinstance(delta, bool) or not isinstance(delta, (int, float)) or not (0.0 < float(delta) < float("inf")):
        raise ValueError("%s: robust=dict(delta=%r) must be a finite number > 0" % (what, delta))
    edges = robust.get("edges", ("loop",))
    edges = (edges,) if isinstance(edges, str) else tuple(edges)
    if not edges or any(not isinstance(e, str) or e not in EDGE_CLASSES for e in edges) or len(set(edges)) != len(edges):
        raise ValueError("%s: robust=dict(edges=%r): a non-empty choice of %s, each once" % (what, edges, sorted(EDGE_CLASSES)))
    return ROBUST_KERNELS[name], float(delta), sum(EDGE_CLASSES[e] for e in edges)


def _information(what, kind, i, j, information):
    if information is None:
        return default_information(kind, i, j)
    om = np.array(information.detach().cpu().numpy() if isinstance(information, torch.Tensor) else information,
                  dtype=np.float64)
    if om.shape != (6, 6) or not np.all(np.isfinite(om)) or not np.array_equal(om, om.T):
        raise ValueError("%s: information must be a finite symmetric 6 x 6 matrix" % what)
    return om


def _transform(what, T):
    t = np.array(T.detach().cpu().numpy() if isinstance(T, torch.Tensor) else T, dtype=np.float64)
    if t.shape != (4, 4) or not np.all(np.isfinite(t)):
        raise ValueError("%s: the measurement must be a finite 4 x 4 transform" % what)
    return t


class PoseGraph(Replayed):
    """S pose graphs on the device, one per stream.

    ``append(rel, active=None, valid=None)``: one vertex per stream and call: ``X_k = X_{k-1} . rel`` with the current,
    possibly already optimised ``X_{k-1}``, and the odometry edge ``k-1 -> k`` with ``rel`` as its measurement.  ``active`` /
    ``valid`` (S,) int32 device words as ``StreamingOdometry`` keeps them: a stream with ``active == 0`` keeps every bit, one
    with ``active`` and ``valid == 0`` starts an empty graph (vertex 0 alone).  A vertex beyond ``max_poses`` sets
    ``overflowed()`` and writes nothing.

    ``add_loop(stream, i, j, T, information=None)`` / ``add_absolute(stream, i, T, information=None)`` take host integers;
    the few long-range edges and their per-vertex incidence lists are kept on the host and rewritten into static device
    buffers, so a captured ``optimize`` honours them without a new capture.  Refused with ValueError, before anything is
    written: ``i >= j``, an index beyond the stream's count, a full edge list, a non-symmetric or non-finite information.

    ``optimize(iters=None)``: ``iters`` Levenberg-Marquardt iterations (4 launches each, one more to begin), replayed as
    one graph (another ``iters`` captures again).  A stream freezes with a status bit: CONVERGED (an
    accepted step that lowered chi2 by at most 1e-9 of it, or a gradient below 1e-12), TRIVIAL (a chain without loop or
    absolute edge: chi2 = 0, nothing moves), NONFINITE (chi2 is not finite).  ``active`` there: (S,) int32 device mask or
    None; idle streams keep vertices, edges, lambda and status.

    ``robust=dict(kernel="huber" | "geman_mcclure" | "dcs", delta=1.0, edges=("loop",))`` (section 25.1; also
    ``set_robust``): every edge of the classes in ``edges`` ("chain", "loop", "absolute") contributes rho(c) of its raw term
    ``c = e^T Omega e`` to chi2 and carries the weight ``w = rho'(c)`` on its blocks and gradients; one kind and one delta
    per object (for "dcs" delta is Phi).  ``None`` (the default): no kernel, the launches and bits of a graph without one.
    ``edge_weights()`` reads out ``(c, w)`` of every loop and absolute edge at the vertices as they stand.

    Views (device tensors): ``poses()`` / ``relative_poses()`` (max count, S, 4, 4), or ``stream=i``: (count_i, 4, 4);
    ``chi2()``, ``status()`` (S,); ``diagnostics()``: dict of lam, nu, count, pcg_used, relres, accepted."""

    def __init__(self, streams, max_poses=4096, max_loops=256, max_absolute=256, iters=20, pcg_iters=None, pcg_tol=1e-8,
                 fix_first=True, graph=True, device="cuda", robust=None):
        S, N, ML, MA = stream_count("PoseGraph", streams, MAX_STREAMS), int(max_poses), int(max_loops), int(max_absolute)
        if N < 1 or ML < 1 or MA < 1:
            raise ValueError("PoseGraph: max_poses=%d, max_loops=%d and max_absolute=%d must be >= 1" % (N, ML, MA))
        need_iters("PoseGraph", iters)
        pcg_iters = 12 * N if pcg_iters is None else int(pcg_iters)
        if pcg_iters < 1 or not 0.0 <= float(pcg_tol) < 1.0:
            raise ValueError("PoseGraph: pcg_iters=%d must be >= 1 and pcg_tol=%r in [0, 1)" % (pcg_iters, pcg_tol))
        self.streams, self.max_poses, self.max_loops, self.max_absolute = S, N, ML, MA
        self.iters, self.pcg_iters, self.pcg_tol = int(iters), pcg_iters, float(pcg_tol)
        self.fix_first, self.graph = bool(fix_first), bool(graph)
        self._robust = robust_settings(robust)
        self.device = torch.device(device)
        self.replay = Replay(graph)
        self._alloc()

    # ---- state -------------------------------------------------------------------------------------------------------

    def _alloc(self):
        S, N, ML, MA, dev = self.streams, self.max_poses, self.max_loops, self.max_absolute, self.device
        _lib.load()
        f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
        eye = lambda *s: torch.eye(4, dtype=torch.float64, device=dev).expand(*s, 4, 4).contiguous()
        E = N + ML + MA
        self.bufs = dict(
            X=eye(N, S), Xt=eye(N, S), Zc=eye(N, S), count=torch.ones(S, dtype=torch.int32, device=dev), epoch=i32(S),
            overflow=i32(1), nloops=i32(S), nabs=i32(S), loop_ij=i32(S, ML, 2), loop_Z=eye(S, ML), loop_Om=f64(S, ML, 6, 6),
            abs_i=i32(S, MA), abs_G=eye(S, MA), abs_Om=f64(S, MA, 6, 6), inc_ptr=i32(S, N + 1), inc_ent=i32(S, 2 * ML + MA),
            slots=f64(S, E, SLOT), chi_new=f64(S, E), work=f64(S * N * WORK_PER_VERTEX), delta=f64(S, N, 6), lam=f64(S),
            nu=f64(S), chi2=f64(S), status=i32(S), active=torch.ones(S, dtype=torch.int32, device=dev),
            pcg_used=i32(S, self.iters), relres=f64(S, self.iters), accepted=i32(S, self.iters),
            weights=f64(S, ML + MA, 2))
        self._loops = [[] for _ in range(S)]          # host: (i, j) per stream, in edge order
        self._abs = [[] for _ in range(S)]
        self._epoch = [0] * S

    def _sync_stream(self, s):
        """The stream's count as the device has it now; drops the host's edge lists where the device emptied the graph."""
        words = torch.stack([self.bufs["count"][s], self.bufs["epoch"][s]]).cpu()
        if int(words[1]) != self._epoch[s]:
            self._epoch[s] = int(words[1])
            self._loops[s], self._abs[s] = [], []
        return int(words[0])

    def _write_incidence(self, s):
        N, ML = self.max_poses, self.max_loops
        inc = {}
        for l, (i, j) in enumerate(self._loops[s]):
            inc.setdefault(i, []).append((N + l) * 2)
            inc.setdefault(j, []).append((N + l) * 2 + 1)
        for a, i in enumerate(self._abs[s]):
            inc.setdefault(i, []).append((N + ML + a) * 2 + 1)
        ptr = np.zeros(N + 1, dtype=np.int32)
        ent = np.zeros(2 * ML + self.max_absolute, dtype=np.int32)
        at = 0
        for v in sorted(inc):
            ptr[v + 1] = len(inc[v])
            ent[at:at + len(inc[v])] = inc[v]
            at += len(inc[v])
        np.cumsum(ptr, out=ptr)
        self.bufs["inc_ptr"][s].copy_(torch.from_numpy(ptr))
        self.bufs["inc_ent"][s].copy_(torch.from_numpy(ent))

    def add_loop(self, stream, i, j, T, information=None):
        s = stream_index(None, "add_loop", stream, self.streams)
        i, j = int(i), int(j)
        Z = _transform("add_loop", T)
        om = _information("add_loop", "loop", i, j, information)
        n = self._sync_stream(s)
        if not 0 <= i < j:
            raise ValueError("add_loop: i=%d, j=%d must satisfy 0 <= i < j" % (i, j))
        if j >= n:
            raise ValueError("add_loop: j=%d beyond the %d poses of stream %d" % (j, n, s))
        l = len(self._loops[s])
        if l >= self.max_loops:
            raise ValueError("add_loop: stream %d already holds max_loops=%d loop edges" % (s, self.max_loops))
        b = self.bufs
        self._loops[s].append((i, j))
        b["loop_ij"][s, l].copy_(torch.tensor([i, j], dtype=torch.int32))
        b["loop_Z"][s, l].copy_(torch.from_numpy(Z))
        b["loop_Om"][s, l].copy_(torch.from_numpy(om))
        self._write_incidence(s)
        b["nloops"][s:s + 1].fill_(l + 1)

    def add_absolute(self, stream, i, T, information=None):
        s = stream_index(None, "add_absolute", stream, self.streams)
        i = int(i)
        G = _transform("add_absolute", T)
        om = _information("add_absolute", "absolute", i, i, information)
        n = self._sync_stream(s)
        if not 0 <= i < n:
            raise ValueError("add_absolute: i=%d outside the %d poses of stream %d" % (i, n, s))
        a = len(self._abs[s])
        if a >= self.max_absolute:
            raise ValueError("add_absolute: stream %d already holds max_absolute=%d edges" % (s, self.max_absolute))
        b = self.bufs
        self._abs[s].append(i)
        b["abs_i"][s, a:a + 1].fill_(i)
        b["abs_G"][s, a].copy_(torch.from_numpy(G))
        b["abs_Om"][s, a].copy_(torch.from_numpy(om))
        self._write_incidence(s)
        b["nabs"][s:s + 1].fill_(a + 1)

    def set_robust(self, robust):
        """Another kernel, delta or choice of classes (or None: none) from the next ``optimize`` on, for every edge of
        those classes.  A captured ``optimize`` holds the old settings in its launches, so it is dropped and the next
        call captures again."""
        new = robust_settings(robust, "set_robust")
        if new != self._robust:
            self._robust = new
            self.replay.drop()

    def robust(self):
        """The settings in force: None or (kind, delta, edge mask)."""
        return self._robust

    def reset(self, streams=None):
        """Empties the graphs of ``streams`` (host indices; None: all): vertex 0 alone, no edges, status 0."""
        b = self.bufs
        for s in stream_indices(None, "reset", streams, self.streams):
            self._loops[s], self._abs[s] = [], []
            for name in ("nloops", "nabs", "status"):
                b[name][s:s + 1].zero_()
            for name in ("lam", "nu", "chi2"):
                b[name][s:s + 1].zero_()
            b["count"][s:s + 1].fill_(1)
            b["X"][0, s].copy_(torch.eye(4, dtype=torch.float64))
            self._write_incidence(s)
        if streams is None:
            b["overflow"].zero_()

    # ---- launches ----------------------------------------------------------------------------------------------------

    def _mask(self, what, m):
        if m is not None:
            _need(m, "%s: mask" % what, torch.int32, (self.streams,))
        return m

    def append(self, rel, active=None, valid=None, count=None):
        """``count`` (S,) int32: the stream engine's frame counters after its own append; the vertex is then ``count - 1``,
        which must be the graph's next one (anything else sets the overflow word and writes nothing)."""
        S, b = self.streams, self.bufs
        self._mask("append", active), self._mask("append", valid), self._mask("append", count)
        if isinstance(rel, torch.Tensor) and rel.dtype == torch.float32:
            _need(rel, "append: rows", torch.float32, (S, 7))
            mats, rows = None, rel
        else:
            _need(rel, "append: rel", torch.float64, (S, 4, 4))
            mats, rows = rel, None
        _lib.call("pose_graph_append_kernel_wrapper", self.device, S, self.max_poses, _p(active), _p(valid), _p(count),
                  _p(mats), _p(rows), _p(b["X"]), _p(b["Zc"]), _p(b["count"]), _p(b["nloops"]), _p(b["nabs"]), _p(b["epoch"]),
                  _p(b["overflow"]))

    def _graph_args(self):
        return (self.streams, self.max_poses, self.max_loops, self.max_absolute)

    def linearise(self, trial=False):
        """One launch: the slots at the vertices, or (``trial=True``) the chi2 terms at the trial poses."""
        b = self.bufs
        graph = (_p(b["active"]), _p(b["status"]), _p(b["count"]), _p(b["nloops"]), _p(b["nabs"]),
                 _p(b["Xt"] if trial else b["X"]), _p(b["Zc"]), _p(b["loop_ij"]), _p(b["loop_Z"]), _p(b["loop_Om"]),
                 _p(b["abs_i"]), _p(b["abs_G"]), _p(b["abs_Om"]), 0 if trial else _p(b["slots"]),
                 _p(b["chi_new"]) if trial else 0)
        if self._robust is None:
            _lib.call("pose_graph_linearise_kernel_wrapper", self.device, *self._graph_args(), *graph)
        else:
            kind, delta, mask = self._robust
            _lib.call("pose_graph_linearise_robust_kernel_wrapper", self.device, *self._graph_args(), kind, mask, delta,
                      *graph)

    def solve(self, it=0):
        b = self.bufs
        _lib.call("pose_graph_solve_kernel_wrapper", self.device, *self._graph_args(), int(self.fix_first), int(it),
                  self.pcg_iters, self.pcg_tol, _p(b["active"]), _p(b["status"]), _p(b["count"]), _p(b["nloops"]),
                  _p(b["nabs"]), _p(b["loop_ij"]), _p(b["abs_i"]), _p(b["inc_ptr"]), _p(b["inc_ent"]), _p(b["slots"]),
                  _p(b["X"]), _p(b["work"]), _p(b["delta"]), _p(b["Xt"]), _p(b["lam"]), _p(b["nu"]), _p(b["chi2"]),
                  _p(b["pcg_used"]), _p(b["relres"]), b["pcg_used"].shape[1])

    def retract(self):
        """Xt = X . D(delta) for the vertices in use (the last step of ``solve``, alone)."""
        b = self.bufs
        _lib.call("pose_graph_retract_kernel_wrapper", self.device, self.streams, self.max_poses, int(self.fix_first),
                  _p(b["active"]), _p(b["status"]), _p(b["count"]), _p(b["X"]), _p(b["delta"]), _p(b["Xt"]))

    def judge(self, it=0):
        b = self.bufs
        _lib.call("pose_graph_judge_kernel_wrapper", self.device, *self._graph_args(), int(self.fix_first), int(it),
                  _p(b["active"]), _p(b["status"]), _p(b["count"]), _p(b["nloops"]), _p(b["nabs"]), _p(b["loop_ij"]),
                  _p(b["abs_i"]), _p(b["inc_ptr"]), _p(b["inc_ent"]), _p(b["slots"]), _p(b["chi_new"]), _p(b["delta"]),
                  _p(b["Xt"]), _p(b["X"]), _p(b["lam"]), _p(b["nu"]), _p(b["chi2"]), _p(b["accepted"]),
                  b["accepted"].shape[1])

    def begin(self, iters):
        b = self.bufs
        _lib.call("pose_graph_begin_kernel_wrapper", self.device, self.streams, int(iters), b["pcg_used"].shape[1],
                  _p(b["active"]), _p(b["count"]), _p(b["nloops"]), _p(b["nabs"]), _p(b["status"]), _p(b["pcg_used"]),
                  _p(b["relres"]), _p(b["accepted"]), _p(b["chi2"]))

    def _body(self, iters):
        self.begin(iters)
        for it in range(iters):
            self.linearise()
            self.solve(it)
            self.linearise(trial=True)
            self.judge(it)

    def optimize(self, iters=None, active=None):
        iters = self.iters if iters is None else int(iters)
        if not 1 <= iters <= self.iters:
            raise ValueError("optimize: iters=%d outside [1, %d] (the constructor's iters sizes the diagnostics)"
                             % (iters, self.iters))
        b = self.bufs
        if active is None:
            b["active"].fill_(1)
        else:
            b["active"].copy_(self._mask("optimize", active))
        if self.replay.graph(iters) is None:                # one graph at a time: another iters replaces the one held
            self.replay.drop()
        self.replay.run(lambda: self._body(iters), self.device, iters)

    # ---- views -------------------------------------------------------------------------------------------------------

    def _view(self, buf, stream):
        counts = self.bufs["count"]
        if stream is None:
            return buf[:int(counts.max())]
        s = stream_index(None, "poses", stream, self.streams)
        return buf[:int(counts[s]), s]

    def poses(self, stream=None):
        return self._view(self.bufs["X"], stream)

    def relative_poses(self, stream=None):
        return self._view(self.bufs["Zc"], stream)

    def counts(self):
        return self.bufs["count"]

    def chi2(self):
        return self.bufs["chi2"]

    def status(self):
        return self.bufs["status"]

    def edge_weights(self, stream=None):
        """One launch at the vertices as they stand, idle and frozen streams included -> (loops (S, max_loops, 2),
        absolutes (S, max_absolute, 2)) fp64 device views, or with ``stream=i`` that stream's (max_loops, 2) and
        (max_absolute, 2): per edge the raw ``c = e^T Omega e`` and the weight ``w`` its class's kernel gives it (1 without
        one); zeros past the edges in use."""
        b = self.bufs
        kind, delta, mask = (0, 0.0, 0) if self._robust is None else self._robust
        _lib.call("pose_graph_edge_weights_kernel_wrapper", self.device, *self._graph_args(), kind, mask, delta,
                  _p(b["nloops"]), _p(b["nabs"]), _p(b["X"]), _p(b["loop_ij"]), _p(b["loop_Z"]), _p(b["loop_Om"]),
                  _p(b["abs_i"]), _p(b["abs_G"]), _p(b["abs_Om"]), _p(b["weights"]))
        loops, absolutes = b["weights"][:, :self.max_loops], b["weights"][:, self.max_loops:]
        if stream is None:
            return loops, absolutes
        s = stream_index(None, "edge_weights", stream, self.streams)
        return loops[s], absolutes[s]

    def loop_weights(self, stream):
        """(nloops, 2): ``(c, w)`` of the stream's loops in use, in the order they were added."""
        s = stream_index(None, "loop_weights", stream, self.streams)
        return self.edge_weights(s)[0][:int(self.bufs["nloops"][s])]

    def overflowed(self):
        return bool(self.bufs["overflow"].item())

    def diagnostics(self):
        b = self.bufs
        return {k: b[k] for k in ("lam", "nu", "count", "pcg_used", "relres", "accepted", "nloops", "nabs")}
