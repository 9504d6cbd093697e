"""Localisation of a frame in the global map: point-to-plane ICP of a cloud against the voxel-hashed
world map of ``global_map.GlobalMap``, the plane of every pair fitted from the map's own neighbourhood.

    gm = GlobalMap(streams=S, num_points=8192, voxel_size=0.3)
    ...                                      # gm.advance(...) per frame, gm.rebuild(...) after a loop closure
    loc = MapLocalizer(gm)
    loc.index()                              # slot -> rank of the map as it stands (index(full=False): only the new ranks)
    T = loc.localize(cloud, guess)           # (S, 4, 4) fp64: the cloud's pose in the map's world frame

The rule (``tests/map_localize_model.py`` is it in NumPy): a query ``q = float32(T p)`` lies in the voxel ``c = rint(q /
v)``; the candidates are the map's points of the ``(2 R + 1)^3`` voxels around ``c`` in dz, dy, dx order; the pair is the
nearest of them (fp32 distance, the first on a tie), its plane the smallest eigenvector of the covariance of all
candidates about their mean.  Nothing of the map is written.  The kernels are ``csrc/map_localize.hip``; the solver is the
refiners' (``icp_solve_masked_kernel_wrapper``).  There is no CPU path.
"""
import numpy as np
import torch

from . import _lib, evaluation, stream_masks
from .global_map import GlobalMap
from .registration import ROW, groups
from .stream_engine import need as _need, ptr as _p
from .stream_engine import Replay, Replayed, init_poses, need_cuda, need_iters, need_sigma, need_solver

MAX_STREAMS = 1024                               # csrc/map_localize.hip: ML_MAX_STREAMS
NO_PLANE = (1 << 31) - 1                         # min_neighbours of ``lookup``: no neighbourhood is that large


def index_bytes(S, T):
    """Bytes of the index of S streams over tables of T slots: ``4 (T + 1)`` each."""
    return int(S) * 4 * (int(T) + 1)


def largest_max_dist(radius, voxel_size):
    """The largest fp32 number that is <= radius * voxel_size: what ``max_dist=None`` means."""
    bound = float(radius) * float(voxel_size)
    f = np.float32(bound)
    if float(f) > bound:
        f = np.nextafter(f, np.float32(0.0))
    return float(f)


def _need_radius(what, radius):
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or int(radius) not in (1, 2):
        raise ValueError("%s: radius=%r must be 1 or 2" % (what, radius))
    return int(radius)


def _need_voxel(what, voxel_size):
    ok = isinstance(voxel_size, (int, float, np.integer, np.floating)) and not isinstance(voxel_size, bool)
    if not ok or not np.isfinite(float(voxel_size)) or not float(voxel_size) > 0.0:
        raise ValueError("%s: voxel_size=%r must be finite and > 0" % (what, voxel_size))
    return float(voxel_size)


def _need_max_dist(what, max_dist, radius, voxel_size):
    """-> max_dist as the fp32 number the kernel compares with; None: the largest that the block of voxels allows."""
    if max_dist is None:
        return largest_max_dist(radius, voxel_size)
    ok = isinstance(max_dist, (int, float, np.integer, np.floating)) and not isinstance(max_dist, bool)
    if not ok or not 0.0 <= float(max_dist) <= radius * voxel_size:
        raise ValueError("%s: max_dist=%r outside [0, radius * voxel_size = %r] (the %d voxels around a query hold every map "
                         "point that near)" % (what, max_dist, radius * voxel_size, (2 * radius + 1) ** 3))
    f = np.float32(max_dist)                         # the bound itself may round up to fp32: then the fp32 number below it
    return float(f) if float(f) <= radius * voxel_size else float(np.nextafter(f, np.float32(0.0)))


def _need_min_neighbours(what, k):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or int(k) < 1:
        raise ValueError("%s: min_neighbours=%r must be an integer >= 1" % (what, k))
    return int(k)


def _need_map(what, keys, rows, points, source, total, index):
    """The map's buffers and the index -> (S, T, capacity)."""
    if not isinstance(keys, torch.Tensor) or keys.dim() != 2:
        raise ValueError("%s: keys must be int64 (S, T)" % what)
    S, T = int(keys.shape[0]), int(keys.shape[1])
    if not 1 <= S <= MAX_STREAMS:
        raise ValueError("%s: S=%d outside [1, %d]" % (what, S, MAX_STREAMS))
    if T < 64 or T > 1 << 30 or T & (T - 1):
        raise ValueError("%s: T=%d must be a power of two in [2^6, 2^30]" % (what, T))
    if not isinstance(points, torch.Tensor) or points.dim() != 3 or points.shape[1] < 1:
        raise ValueError("%s: points must be float32 (S, capacity >= 1, 3)" % what)
    cap = int(points.shape[1])
    _need(keys, "%s: keys" % what, torch.int64, (S, T), cuda=False)
    _need(rows, "%s: rows" % what, torch.int32, (S, T + 2), cuda=False)
    _need(points, "%s: points" % what, torch.float32, (S, cap, 3), cuda=False)
    _need(source, "%s: source" % what, torch.int32, (S, cap, 2), cuda=False)
    if not isinstance(total, torch.Tensor) or total.dtype != torch.int32 or tuple(total.shape) != (S,):
        raise ValueError("%s: total must be an int32 tensor of shape (%d,), got %s %s"
                         % (what, S, getattr(total, "dtype", type(total)), tuple(getattr(total, "shape", ()))))
    if S > 1 and total.stride(0) < 1:
        raise ValueError("%s: total must have a positive stride" % what)
    _need(index, "%s: index" % what, torch.int32, (S, T + 1), cuda=False)
    return S, T, cap


def _map_args(keys, points, source, total):
    return _p(keys), _p(points), _p(source), _p(total), int(total.stride(0)) if total.shape[0] > 1 else 1


def new_index(S, T, device):
    """An index that knows nothing: (S, T + 1) int32 of -1."""
    assert _lib.load().map_localize_index_bytes(S, T) == index_bytes(S, T)
    return torch.full((S, T + 1), -1, dtype=torch.int32, device=device)


# ---- the ops alone -----------------------------------------------------------------------------------------------------

def index(keys, rows, points, source, total, voxel_size, index=None, indexed=None, full=True):
    """One index pass over the map's buffers (``GlobalMap.bufs``: keys (S, T) int64, rows (S, T + 2) int32, points (S,
    capacity, 3) fp32, source (S, capacity, 2) int32; total (S,) int32, ``GlobalMap.totals()``) -> (index (S, T + 1) int32,
    indexed (S,) int32), in place where they are given.  ``full``: ranks [0, M); else [indexed[s], M).  ``rows`` is taken for
    the signature's sake and its shape checked; no kernel reads it (the validation of an entry makes it unnecessary)."""
    what = "map_localize.index"
    voxel_size = _need_voxel(what, voxel_size)
    if index is None and isinstance(keys, torch.Tensor) and keys.dim() == 2 and keys.is_cuda:
        index = torch.full((keys.shape[0], keys.shape[1] + 1), -1, dtype=torch.int32, device=keys.device)
    S, T, cap = _need_map(what, keys, rows, points, source, total, index)
    if indexed is None:
        indexed = torch.zeros((S,), dtype=torch.int32, device=keys.device)
    _need(indexed, "%s: indexed" % what, torch.int32, (S,), cuda=False)
    need_cuda(keys, rows, points, source, total, index, indexed)
    _lib.call("map_index_kernel_wrapper", keys.device, S, T, cap, voxel_size, *_map_args(keys, points, source, total),
              1 if full else 0, 0, _p(indexed), _p(index))
    return index, indexed


def accumulate(keys, rows, points, source, total, index, voxel_size, p, T=None, radius=1, sigma=0.5, max_dist=None,
               min_neighbours=5, max_source_frame=None, active=None, nearest=False):
    """One launch of the hot path -> partial (S, groups(n), 32) fp64 in ``registration.solve``'s layout.  p (S, n, 3) fp32; T
    (S, 4, 4) fp64 the cloud's pose estimate in the world frame (None: p are world points and the sensor is the origin).
    ``max_source_frame`` (S,) int32: only map points of frames up to it are candidates.  ``active`` (S,) int32: idle streams
    get zero rows.  ``nearest=True`` -> (partial, rank, count, dist, normal): per point the nearest candidate's rank (-1:
    none), the number of candidates, the fp32 distance (+Inf: none) and the fitted plane's normal (zero: none fitted).
    ``rows`` is not read (see ``index``)."""
    what = "map_localize.accumulate"
    voxel_size, radius = _need_voxel(what, voxel_size), _need_radius(what, radius)
    need_sigma(what, sigma)
    max_dist = _need_max_dist(what, max_dist, radius, voxel_size)
    min_neighbours = _need_min_neighbours(what, min_neighbours)
    S, Tn, cap = _need_map(what, keys, rows, points, source, total, index)
    if not isinstance(p, torch.Tensor) or p.dim() != 3 or p.shape[1] < 1:
        raise ValueError("%s: p must be float32 (S, n >= 1, 3), got %s" % (what, tuple(getattr(p, "shape", ()))))
    n = int(p.shape[1])
    _need(p, "%s: p" % what, torch.float32, (S, n, 3), cuda=False)
    if T is not None:
        _need(T, "%s: T" % what, torch.float64, (S, 4, 4), cuda=False)
    for name, m in (("max_source_frame", max_source_frame), ("active", active)):
        if m is not None:
            _need(m, "%s: %s" % (what, name), torch.int32, (S,), cuda=False)
    need_cuda(keys, rows, points, source, total, index, p, T, max_source_frame, active)
    dev = p.device
    partial = torch.empty((S, groups(n), ROW), dtype=torch.float64, device=dev)
    rank = count = dist = normal = None
    if nearest:                                      # an idle stream's rows are not written, so they start defined
        rank = torch.full((S, n), -1, dtype=torch.int32, device=dev)
        count = torch.zeros((S, n), dtype=torch.int32, device=dev)
        dist = torch.full((S, n), float("inf"), dtype=torch.float32, device=dev)
        normal = torch.zeros((S, n, 3), dtype=torch.float32, device=dev)
    _lib.call("map_localize_accumulate_kernel_wrapper", dev, S, n, Tn, cap, voxel_size, radius,
              *_map_args(keys, points, source, total), _p(index), _p(p), _p(T), _p(max_source_frame), float(sigma), max_dist,
              min_neighbours, _p(partial), _p(rank), _p(count), _p(dist), _p(normal), _p(active))
    return (partial, rank, count, dist, normal) if nearest else partial


def lookup(keys, rows, points, source, total, index, voxel_size, q, radius, max_source_frame=None, active=None):
    """-> (rank, count, dist), each (S, n): for every world point of q (S, n, 3) fp32 the nearest candidate among the (2
    radius + 1)^3 voxels around it, the number of candidates and the fp32 distance; (-1, count, +Inf) where there is none.
    No distance bound and no plane: those are the pair's.  ``rows`` is not read (see ``index``)."""
    return accumulate(keys, rows, points, source, total, index, voxel_size, q, None, radius, 1.0, None, NO_PLANE,
                      max_source_frame, active, nearest=True)[1:4]


# ---- the localiser -----------------------------------------------------------------------------------------------------

class MapLocalizer(Replayed):
    """Localises one cloud per call and stream in the stream's global map.

    ``index(full=True)``: the index pass over the map as it stands (two launches; ``full=False``: only the ranks that came
    since the last pass, what an ``advance`` appended).  After ``GlobalMap.rebuild`` index in full: until then a lookup
    finds the new map's point of a voxel or nothing, never another point.

    ``localize(cloud, init, active=None, max_source_frame=None, trace=False)``: cloud (S, n, 3) fp32; init (S, 4, 4) fp64
    or (S, 7) fp32 pose rows, the guess of the cloud's pose in the map's world frame -> the refined pose (S, 4, 4) fp64, a
    static buffer that the next call overwrites.  ``iters`` Gauss-Newton iterations always run and streams freeze on the
    device as ``registration.IcpRefiner``'s do (``status()``: 1 converged, 2 fewer than ``min_pairs`` pairs, 4 pivot, 8
    idle; a stream frozen in iteration 0 returns ``init`` bit for bit).  ``active``: a mask as the refiners take it; an idle
    stream keeps every word of its pose.  ``max_source_frame`` (S,) int32, device tensor or host integers: only map points
    of frames up to it attract.  One call is ``1 + 2 iters`` launches (begin; accumulate and solve per iteration) with no
    allocation and no sync, replayed as one graph keyed by the map's buffers.  ``trace=True``
    (``graph=False`` only) also returns per iteration clones of rank, count, dist, normal, the summed row, delta and T.

    ``max_dist=None``: the largest fp32 number <= ``radius * voxel_size``; a larger one is refused, because the block of
    voxels would no longer hold every map point that near.  ``indexed()``: (S,) int32 device view of the ranks the index
    covers.  ``index_bytes()``: ``4 (T + 1)`` per stream."""

    _name = "MapLocalizer"

    def __init__(self, global_map, iters=10, sigma=0.5, max_dist=None, radius=1, min_neighbours=5, damping=1e-6,
                 threshold_delta_pose=1e-4, min_pairs=64, graph=True):
        what = self._name
        if not isinstance(global_map, GlobalMap):
            raise ValueError("%s: global_map must be a GlobalMap, got %s" % (what, type(global_map).__name__))
        self.map = global_map
        self.streams, self.voxel_size = global_map.streams, global_map.voxel_size
        if self.streams > MAX_STREAMS:
            raise ValueError("%s: streams=%d outside [1, %d]" % (what, self.streams, MAX_STREAMS))
        need_iters(what, iters)
        need_sigma(what, sigma)
        self.radius = _need_radius(what, radius)
        self.max_dist = _need_max_dist(what, max_dist, self.radius, self.voxel_size)
        self.min_neighbours = _need_min_neighbours(what, min_neighbours)
        need_solver(what, damping, threshold_delta_pose, min_pairs)
        self.iters, self.sigma, self.damping = int(iters), float(sigma), float(damping)
        self.threshold_delta_pose, self.min_pairs, self.graph = float(threshold_delta_pose), int(min_pairs), bool(graph)
        self.replay, self.index_replay = Replay(graph), Replay(graph)
        self.bufs = None
        self.num_points = None

    # ---- state -------------------------------------------------------------------------------------------------------

    def _map(self):
        m = self.map.bufs
        if m is None:
            raise ValueError("%s: the GlobalMap has no buffers yet (advance or rebuild it first)" % self._name)
        return m

    def _alloc(self):
        m, S = self._map(), self.streams
        dev = m["keys"].device
        T = int(m["keys"].shape[1])
        f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
        eye = torch.eye(4, dtype=torch.float64, device=dev).expand(S, 4, 4).contiguous()
        self.bufs = dict(index=new_index(S, T, dev), indexed=i32(S), init=eye.clone(), T=eye, status=i32(S),
                         iterations=i32(S), pairs=i32(S), cost=f64(S), sum=f64(S, ROW), delta=f64(S, 6),
                         active=torch.ones(S, dtype=torch.int32, device=dev), newest=i32(S))

    def _table(self):
        """What every launch takes of the map: (T, capacity, voxel, keys, points, source, total, stride)."""
        m = self._map()
        return (int(m["keys"].shape[1]), self.map.capacity, self.voxel_size, _p(m["keys"]), _p(m["points"]), _p(m["source"]),
                m["state"].data_ptr() + 8, int(m["state"].shape[1]))          # the total word: state[s][2]

    def index_bytes(self):
        return index_bytes(self.streams, int(self._map()["keys"].shape[1]))

    def indexed(self):
        """(S,) int32 device view: the ranks [0, indexed) are in the index.  None before the first pass."""
        return None if self.bufs is None else self.bufs["indexed"]

    def status(self):
        """(S,) int32 device view of the last ``localize``: 0 moved in every iteration, else why the stream froze."""
        return None if self.bufs is None else self.bufs["status"]

    def diagnostics(self):
        """Device views of the last ``localize``: iterations used, pairs and the weighted cost of the last iteration a
        stream took part in."""
        if self.bufs is None:
            return None
        return dict(iterations=self.bufs["iterations"], pairs=self.bufs["pairs"], cost=self.bufs["cost"])

    # ---- launches ----------------------------------------------------------------------------------------------------

    def index(self, full=True, refill=None):
        """``refill`` (S,) int32 device word, with ``full=False``: the streams whose word is set are indexed from rank 0
        (their map was emptied since the last pass); the graph reads the word, so keep passing the same tensor."""
        if refill is not None:
            _need(refill, "%s: refill" % self._name, torch.int32, (self.streams,))
        if self.bufs is None:
            self._alloc()
        b, table = self.bufs, self._table()
        dev = b["index"].device

        def body():
            _lib.call("map_index_kernel_wrapper", dev, self.streams, *table, 1 if full else 0, _p(refill), _p(b["indexed"]),
                      _p(b["index"]))
        self.index_replay.run(body, dev, (bool(full), _p(refill)) + table)

    def _body(self, gated, trace=None):
        b, S, n = self.bufs, self.streams, self.num_points
        dev, table, G = b["index"].device, self._table(), b["partial"].shape[1]
        active = _p(b["active"])
        _lib.call("map_localize_begin_kernel_wrapper", dev, S, _p(b["init"]), active, _p(b["T"]))
        for it in range(self.iters):
            near = [None] * 4
            if trace is not None:
                near = [torch.full((S, n), -1, dtype=torch.int32, device=dev), torch.zeros((S, n), dtype=torch.int32,
                        device=dev), torch.full((S, n), float("inf"), dtype=torch.float32, device=dev),
                        torch.zeros((S, n, 3), dtype=torch.float32, device=dev)]
            _lib.call("map_localize_accumulate_kernel_wrapper", dev, S, n, table[0], table[1], table[2], self.radius,
                      *table[3:], _p(b["index"]), _p(b["cloud"]), _p(b["T"]), _p(b["newest"]) if gated else 0, self.sigma,
                      self.max_dist, self.min_neighbours, _p(b["partial"]), _p(near[0]), _p(near[1]), _p(near[2]),
                      _p(near[3]), active)
            if trace is not None:
                before = b["T"].clone()
            _lib.call("icp_solve_masked_kernel_wrapper", dev, S, G, it, _p(b["partial"]), self.damping,
                      self.threshold_delta_pose, self.min_pairs, _p(b["T"]), _p(b["status"]), _p(b["iterations"]),
                      _p(b["pairs"]), _p(b["cost"]), _p(b["sum"]), _p(b["delta"]), active)
            if trace is not None:
                trace.append(dict(rank=near[0], count=near[1], dist=near[2], normal=near[3], sum=b["sum"].clone(),
                                  delta=b["delta"].clone(), T_before=before, T=b["T"].clone(), status=b["status"].clone()))

    def localize(self, cloud, init, active=None, max_source_frame=None, trace=False):
        what, S = self._name, self.streams
        if trace and self.graph:
            raise ValueError("%s: trace=True needs graph=False (a replayed graph cannot hand out its iterations)" % what)
        if not isinstance(cloud, torch.Tensor) or cloud.dim() != 3 or cloud.shape[1] < 1:
            raise ValueError("%s: cloud must be float32 (%d, n >= 1, 3), got %s" % (what, S, tuple(getattr(cloud, "shape", ()))))
        n = int(cloud.shape[1])
        _need(cloud, "%s: cloud" % what, torch.float32, (S, n, 3), cuda=False)
        init_poses(what, init, S)
        act = None if active is None else stream_masks.stream_mask(active, S, "active", what)
        newest = None
        if max_source_frame is not None:
            if isinstance(max_source_frame, torch.Tensor):
                _need(max_source_frame, "%s: max_source_frame" % what, torch.int32, (S,), cuda=False)
                newest = max_source_frame
            else:
                ids = np.asarray(max_source_frame)
                if ids.shape != (S,) or ids.dtype.kind not in "iu":
                    raise ValueError("%s: max_source_frame must be (%d,) integers" % (what, S))
                newest = torch.from_numpy(ids.astype(np.int32))
        need_cuda(cloud, init)
        self._map()
        if init.dim() == 2:
            init = evaluation.rows_to_transforms(init)
        if self.bufs is None:
            self._alloc()
        b = self.bufs
        if self.num_points != n:                            # another cloud size: its buffers, and graphs of their own
            dev = b["index"].device
            b["cloud"] = torch.zeros((S, n, 3), dtype=torch.float32, device=dev)
            b["partial"] = torch.zeros((S, groups(n), ROW), dtype=torch.float64, device=dev)
            self.num_points = n
            self.replay.drop()
        if act is None:
            b["active"].fill_(1)
        else:
            b["active"].copy_(act)
        b["cloud"].copy_(cloud)
        b["init"].copy_(init)
        gated = newest is not None
        if gated:
            b["newest"].copy_(newest)
        steps = [] if trace else None
        self.replay.run(lambda: self._body(gated, steps), b["index"].device, (gated, n) + self._table())
        return (b["T"], steps) if trace else b["T"]
