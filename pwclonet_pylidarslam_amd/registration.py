"""Point-to-plane registration of incoming frames against a sliding local map, on the device.

The reference's odometry is ``ICPFrameToModel`` (R/slam/odometry/icp_odometry.py:248-299, R = /root/reference): a learned
model supplies the initial guess (R/slam/initialization.py:225-285) and point-to-plane Gauss-Newton refines it against a
local map of the last frames (R/slam/odometry/local_map.py:254-427, R/slam/common/optimization.py:297-354, 391-443), on the
host.  ``IcpRefiner`` does the refinement with the kernels of ``csrc/icp.hip`` and the existing neighbour search:

    ref = IcpRefiner(streams=S, num_points=8192)
    T = ref.register(cloud, init)          # cloud (S, n, 3) fp32, init (S, 4, 4) fp64 or (S, 7) pose rows

``T`` maps the frame's points into the previous frame (``synthetic.kitti_like_sequence``'s ground truth, what
``StreamingOdometry.trajectory()`` multiplies).  Every map slot keeps its cloud, normals and search structure in its own
frame; only the frame's points move (``icp_queries``).  One iteration is four launches (queries, search, accumulate, solve);
the iteration count is fixed and streams freeze on the device (``status()``), so a whole registration plus the map handover
replays as one captured graph.  There is no CPU path.

The registration is masked: two (S,) words in device memory say which streams delivered a frame and which of those start
a new sequence, and one graph serves idle, restarting and pairing streams alike.  An idle stream keeps its map and gets
status ``IDLE``.  ``IcpRefiner(..., per_stream=True)`` lets every call set the words; lock step (the default) is the same
engine with every stream active, seen through a host-side view.
"""
import numpy as np
import torch

from . import _lib, evaluation, stream_masks
from .stream_engine import need as _need, ptr as _p
from .stream_engine import (Replay, Replayed, init_poses, need_cuda, need_iters, need_max_dist, need_sigma, need_solver,
                            stream_count)

MAX_STREAMS = 1024
MAX_SLOTS = 64                                   # csrc/icp.hip: ICP_MAX_SLOTS
ROW = 32                                         # csrc/icp.hpp: ICP_ROW and the offsets inside a row of sums
H0, G0, SW, COST, PAIRS = 0, 21, 27, 28, 29
CONVERGED, FEW_PAIRS, BAD_PIVOT = 1, 2, 4        # status bits
IDLE = 8                                         # masked registration: the stream delivered no frame in this call


def _need_pairing(sigma, max_dist):
    """The check of the ``accumulate`` ops of this module and of ``projective``."""
    if not float(sigma) > 0.0 or not float(max_dist) >= 0.0:
        raise ValueError("accumulate: sigma=%r must be > 0 and max_dist=%r >= 0" % (sigma, max_dist))


def groups(n):
    """Rows of partial sums per stream that ``accumulate`` writes for clouds of n points."""
    return (int(n) + 255) // 256


# ---- the ops alone -----------------------------------------------------------------------------------------------------

def self_neighbours(xyz, k):
    """xyz (b, n, 3) -> (idx (b, n, k + 1) int32 of every point's k + 1 nearest in its own cloud, the structure)."""
    b, n, _ = xyz.shape
    lib = _lib.load()
    ws = torch.empty((lib.knn_point_build_bytes(b, n),), dtype=torch.uint8, device=xyz.device)
    idx = torch.empty((b, n, k + 1), dtype=torch.int32, device=xyz.device)
    _lib.call("knn_build_kernel_wrapper", xyz.device, b, n, _p(xyz), _p(ws), 0)
    _lib.call("knn_point_prebuilt_kernel_wrapper", xyz.device, b, n, n, k + 1, _p(xyz), _p(idx), 0, _p(ws))
    return idx, ws


def normals(xyz, k=10):
    """xyz (b, n, 3) fp32, 64 <= n <= 16384 -> (normals (b, n, 3) fp32, eig (b, n, 3) fp64 ascending): the unit eigenvector
    of the smallest eigenvalue of the covariance of the k nearest neighbours about the point, turned towards the origin;
    zero where that covariance has rank below 2."""
    if not isinstance(xyz, torch.Tensor) or xyz.dim() != 3 or xyz.shape[-1] != 3:
        raise ValueError("normals: xyz must be (b, n, 3), got %s" % (tuple(getattr(xyz, "shape", ())),))
    b, n, _ = xyz.shape
    k = int(k)
    if not 64 <= n <= 16384:
        raise ValueError("normals: n=%d outside [64, 16384] (the neighbour search's range)" % n)
    if not 1 <= k <= min(63, n - 1):
        raise ValueError("normals: k=%d outside [1, %d]" % (k, min(63, n - 1)))
    _need(xyz, "normals: xyz", torch.float32)
    idx, _ = self_neighbours(xyz, k)
    out = torch.empty((b, n, 3), dtype=torch.float32, device=xyz.device)
    eig = torch.empty((b, n, 3), dtype=torch.float64, device=xyz.device)
    _lib.call("icp_normals_kernel_wrapper", xyz.device, b, n, k, _p(xyz), _p(idx), _p(out), _p(eig))
    return out, eig


def _need_mask(active, what, S):
    _need(active, "%s: active" % what, torch.int32, (S,))


def queries(A, p, T=None, active=None, out=None):
    """A (S, M, 4, 4) fp64, p (S, n, 3) fp32, T (S, 4, 4) fp64 or None -> q (S, M, n, 3) = fp32(A[s, m] T[s] p[s, i]).
    ``active`` (S,) int32: the masked launch, which leaves the rows of ``out`` (S, M, n, 3) of idle streams as they are."""
    if not isinstance(A, torch.Tensor) or A.dim() != 4:
        raise ValueError("queries: A must be (S, M, 4, 4)")
    S, M = A.shape[:2]
    _need(A, "queries: A", torch.float64, (S, M, 4, 4))
    if not isinstance(p, torch.Tensor) or p.dim() != 3:
        raise ValueError("queries: p must be (S, n, 3)")
    n = p.shape[1]
    _need(p, "queries: p", torch.float32, (S, n, 3))
    if T is not None:
        _need(T, "queries: T", torch.float64, (S, 4, 4))
    if out is not None:
        _need(out, "queries: out", torch.float32, (S, M, n, 3))
    if out is not None:
        q = out
    else:                                            # masked: idle streams' rows are not written, so they start defined
        q = (torch.empty if active is None else torch.zeros)((S, M, n, 3), dtype=torch.float32, device=p.device)
    if active is None:
        _lib.call("icp_queries_kernel_wrapper", p.device, S, M, n, _p(A), _p(T), _p(p), _p(q))
    else:
        _need_mask(active, "queries", S)
        _lib.call("icp_queries_masked_kernel_wrapper", p.device, S, M, n, _p(A), _p(T), _p(p), _p(q), _p(active))
    return q


def accumulate(p, q, idx, dist, map_xyz, map_normals, live, R, T, sigma=0.5, max_dist=1.0, active=None):
    """One launch of the normal equations' sums -> partial (S, groups(n), 32) fp64, one row per workgroup of 256 points.
    p (S, n, 3), q (S, M, n, 3), idx / dist (S, M, n) from the search with nsample = 1, map_xyz / map_normals (S, M, n, 3),
    live (S, M) int32, R (S, M, 3, 3) and T (S, 4, 4) fp64.  ``active`` (S,) int32: the masked launch, zero rows for idle
    streams."""
    if not isinstance(q, torch.Tensor) or q.dim() != 4:
        raise ValueError("accumulate: q must be (S, M, n, 3)")
    S, M, n, _ = q.shape
    _need_pairing(sigma, max_dist)
    _need(p, "accumulate: p", torch.float32, (S, n, 3))
    _need(q, "accumulate: q", torch.float32, (S, M, n, 3))
    _need(idx, "accumulate: idx", torch.int32, (S, M, n))
    _need(dist, "accumulate: dist", torch.float32, (S, M, n))
    _need(map_xyz, "accumulate: map_xyz", torch.float32, (S, M, n, 3))
    _need(map_normals, "accumulate: map_normals", torch.float32, (S, M, n, 3))
    _need(live, "accumulate: live", torch.int32, (S, M))
    _need(R, "accumulate: R", torch.float64, (S, M, 3, 3))
    _need(T, "accumulate: T", torch.float64, (S, 4, 4))
    partial = torch.empty((S, groups(n), ROW), dtype=torch.float64, device=p.device)
    args = (S, M, n, _p(p), _p(q), _p(idx), _p(dist), _p(map_xyz), _p(map_normals), _p(live), _p(R), _p(T), float(sigma),
            float(max_dist), _p(partial))
    if active is None:
        _lib.call("icp_accumulate_kernel_wrapper", p.device, *args)
    else:
        _need_mask(active, "accumulate", S)
        _lib.call("icp_accumulate_masked_kernel_wrapper", p.device, *args, _p(active))
    return partial


def solve(partial, T, status, it=0, damping=1e-6, threshold_delta_pose=1e-4, min_pairs=64, active=None):
    """One launch of the solver on partial (S, G, 32): updates T (S, 4, 4) fp64 and status (S,) int32 in place and returns
    dict(sum (S, 32), delta (S, 6), iterations, pairs (S,) int32, cost (S,) fp64).  ``active`` (S,) int32: the masked
    launch, which in iteration 0 starts idle streams from status ``IDLE``."""
    if not isinstance(partial, torch.Tensor) or partial.dim() != 3:
        raise ValueError("solve: partial must be (S, G, 32)")
    S, G, _ = partial.shape
    if not float(damping) >= 0.0 or not float(threshold_delta_pose) >= 0.0 or int(min_pairs) < 1 or int(it) < 0:
        raise ValueError("solve: damping, threshold_delta_pose >= 0, min_pairs >= 1 and it >= 0 are required")
    _need(partial, "solve: partial", torch.float64, (S, G, ROW))
    _need(T, "solve: T", torch.float64, (S, 4, 4))
    _need(status, "solve: status", torch.int32, (S,))
    dev = partial.device
    out = dict(sum=torch.empty((S, ROW), dtype=torch.float64, device=dev),
               delta=torch.empty((S, 6), dtype=torch.float64, device=dev),
               iterations=torch.zeros((S,), dtype=torch.int32, device=dev),
               pairs=torch.zeros((S,), dtype=torch.int32, device=dev),
               cost=torch.zeros((S,), dtype=torch.float64, device=dev))
    args = (S, G, int(it), _p(partial), float(damping), float(threshold_delta_pose), int(min_pairs), _p(T), _p(status),
            _p(out["iterations"]), _p(out["pairs"]), _p(out["cost"]), _p(out["sum"]), _p(out["delta"]))
    if active is None:
        _lib.call("icp_solve_kernel_wrapper", dev, *args)
    else:
        _need_mask(active, "solve", S)
        _lib.call("icp_solve_masked_kernel_wrapper", dev, *args, _p(active))
    return out


def begin(active, restart, A, R, live, cursor, armed=None):
    """First launch of a masked registration: the maps of the streams with ``active and (restart or armed)`` are emptied in
    place (live = 0, cursor = 0, A = R = I; ``armed`` is cleared for them).  Masks (S,) int32; A (S, M, 4, 4), R (S, M, 3,
    3) fp64; live (S, M), cursor (S,) int32."""
    if not isinstance(A, torch.Tensor) or A.dim() != 4:
        raise ValueError("begin: A must be (S, M, 4, 4)")
    S, M = A.shape[:2]
    _need_mask(active, "begin", S)
    _need(restart, "begin: restart", torch.int32, (S,))
    if armed is not None:
        _need(armed, "begin: armed", torch.int32, (S,))
    _need(A, "begin: A", torch.float64, (S, M, 4, 4))
    _need(R, "begin: R", torch.float64, (S, M, 3, 3))
    _need(live, "begin: live", torch.int32, (S, M))
    _need(cursor, "begin: cursor", torch.int32, (S,))
    _lib.call("icp_begin_kernel_wrapper", A.device, S, M, _p(active), _p(restart), _p(armed), _p(A), _p(R), _p(live),
              _p(cursor))


def _need_push(what, T, cloud, normals_, stage_ws, map_xyz, map_normals, map_ws, A, R, live, cursor):
    """The argument check of ``map_push`` and ``map_push_keyframe`` -> (S, M, n)."""
    if not isinstance(map_xyz, torch.Tensor) or map_xyz.dim() != 4:
        raise ValueError("%s: map_xyz must be (S, M, n, 3)" % what)
    S, M, n, _ = map_xyz.shape
    lib = _lib.load()
    for t, name, dtype, shape in (
            (T, "T", torch.float64, (S, 4, 4)), (cloud, "cloud", torch.float32, (S, n, 3)),
            (normals_, "normals", torch.float32, (S, n, 3)),
            (stage_ws, "stage_ws", torch.uint8, (lib.knn_point_build_bytes(S, n),)),
            (map_xyz, "map_xyz", torch.float32, (S, M, n, 3)), (map_normals, "map_normals", torch.float32, (S, M, n, 3)),
            (map_ws, "map_ws", torch.uint8, (lib.knn_point_build_bytes(S * M, n),)),
            (A, "A", torch.float64, (S, M, 4, 4)), (R, "R", torch.float64, (S, M, 3, 3)),
            (live, "live", torch.int32, (S, M)), (cursor, "cursor", torch.int32, (S,))):
        _need(t, "%s: %s" % (what, name), dtype, shape)
    return S, M, n


def map_push(T, cloud, normals_, stage_ws, map_xyz, map_normals, map_ws, A, R, live, cursor, active=None):
    """The handover after a registration, in place: the staged frame (cloud, normals (S, n, 3), stage_ws: its structure,
    built for S clouds) goes into slot cursor[s] of map_xyz / map_normals (S, M, n, 3) and map_ws (built for S * M clouds),
    the live slots' A / R are re-based with T (S, 4, 4), the cursor moves on.  ``active`` (S,) int32: the masked launch,
    which leaves idle streams alone."""
    S, M, n = _need_push("map_push", T, cloud, normals_, stage_ws, map_xyz, map_normals, map_ws, A, R, live, cursor)
    args = (S, M, n, _p(T), _p(cloud), _p(normals_), _p(stage_ws), _p(map_xyz), _p(map_normals), _p(map_ws), _p(A), _p(R),
            _p(live), _p(cursor))
    if active is None:
        _lib.call("icp_map_push_kernel_wrapper", T.device, *args)
    else:
        _need_mask(active, "map_push", S)
        _lib.call("icp_map_push_masked_kernel_wrapper", T.device, *args, _p(active))


def map_push_keyframe(T, cloud, normals_, stage_ws, map_xyz, map_normals, map_ws, A, R, live, cursor, insert, active=None):
    """``map_push`` behind the keyframe gate: ``insert`` (S,) int32, the gate's decision.  A stream
    with insert != 0 gets the bits of ``map_push``; one with insert == 0 keeps its slots, ``live`` and ``cursor``, and every
    live slot's A / R is re-based with T.  ``active`` (S,) int32 or None, as there."""
    what = "map_push_keyframe"
    S, M, n = _need_push(what, T, cloud, normals_, stage_ws, map_xyz, map_normals, map_ws, A, R, live, cursor)
    _need(insert, "%s: insert" % what, torch.int32, (S,))
    if active is not None:
        _need_mask(active, what, S)
    _lib.call("keyframe_icp_push_kernel_wrapper", T.device, S, M, n, _p(T), _p(cloud), _p(normals_), _p(stage_ws),
              _p(map_xyz), _p(map_normals), _p(map_ws), _p(A), _p(R), _p(live), _p(cursor), _p(active), _p(insert))


def keyframe_args(what, keyframe):
    """``keyframe=None`` or ``dict(trans=metres, rot=degrees)`` -> None or (trans, rot), both finite and >= 0; ValueError
    naming the argument otherwise."""
    if keyframe is None:
        return None
    if not isinstance(keyframe, dict) or set(keyframe) - {"trans", "rot"}:
        raise ValueError("%s: keyframe=%r must be None or dict(trans=metres, rot=degrees)" % (what, keyframe))
    out = []
    for key, default in (("trans", 0.1), ("rot", 0.3)):             # the reference's threshold_trans / threshold_rot
        v = keyframe.get(key, default)
        ok = isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)
        if not ok or not np.isfinite(float(v)) or float(v) < 0.0:
            raise ValueError("%s: keyframe[%r]=%r must be finite and >= 0" % (what, key, v))
        out.append(float(v))
    return tuple(out)


def keyframe_gate(T, delta, live, trans, rot, active=None, count=None, insert=None):
    """One launch of the keyframe gate, in place on ``delta`` (S, 4, 4) fp64 (the motion since the
    stream's last inserted frame) and ``count`` (S,) int32 (frames inserted since the map was emptied; zeros when None) ->
    (insert (S,) int32, count).  T (S, 4, 4) fp64, live (S, M) int32, ``trans`` metres and ``rot`` degrees, ``active`` (S,)
    int32 or None.  Idle: insert = 0, nothing else changes.  No live slot: insert = 1, delta = I, count = 1.  Otherwise D =
    delta T; insert iff |D[:3, 3]| > trans or the rotation angle of D > rot; insert: delta = I, count += 1; else delta = D."""
    if not isinstance(live, torch.Tensor) or live.dim() != 2:
        raise ValueError("keyframe_gate: live must be (S, M)")
    S, M = live.shape
    trans, rot = keyframe_args("keyframe_gate", dict(trans=trans, rot=rot))
    if not 1 <= S <= MAX_STREAMS or not 1 <= M <= MAX_SLOTS:
        raise ValueError("keyframe_gate: S=%d M=%d out of range (S <= %d, M <= %d)" % (S, M, MAX_STREAMS, MAX_SLOTS))
    _need(T, "keyframe_gate: T", torch.float64, (S, 4, 4))
    _need(delta, "keyframe_gate: delta", torch.float64, (S, 4, 4))
    _need(live, "keyframe_gate: live", torch.int32, (S, M))
    if active is not None:
        _need_mask(active, "keyframe_gate", S)
    if count is None:
        count = torch.zeros((S,), dtype=torch.int32, device=T.device)
    if insert is None:
        insert = torch.zeros((S,), dtype=torch.int32, device=T.device)
    _need(count, "keyframe_gate: count", torch.int32, (S,))
    _need(insert, "keyframe_gate: insert", torch.int32, (S,))
    _lib.call("keyframe_gate_kernel_wrapper", T.device, S, M, _p(T), _p(live), _p(active), trans, rot, _p(delta),
              _p(insert), _p(count))
    return insert, count


# ---- the refiner -------------------------------------------------------------------------------------------------------

class IcpRefiner(Replayed):
    """Registers one frame per call and stream against each stream's map of the last ``map_size`` frames.

    ``register(cloud, init)``: cloud (S, n, 3) fp32, init (S, 4, 4) fp64 or (S, 7) fp32 pose rows [tx ty tz qw qx qy qz]
    (``evaluation.rows_to_transforms``) -> the refined pose (S, 4, 4) fp64, a static buffer that the next call overwrites
    (clone to keep it).  The first frame after a reset only fills the map and returns ``init`` unchanged (no slot is live,
    so the stream freezes in iteration 0 with the few-pairs bit).  ``iters`` Gauss-Newton iterations always run; a stream
    freezes on the device when its step falls below ``threshold_delta_pose`` (status bit 1), when fewer than ``min_pairs``
    points found a partner within ``max_dist`` (bit 2) or when the damped 6x6 system has a pivot that is not positive (bit
    4); a stream frozen by bit 2 or 4 in iteration 0 returns ``init`` bit for bit.  ``damping`` is added to the diagonal of
    the system normalised by the sum of weights: a direction the scene does not constrain keeps the initial guess.
    Edges the kernels pin (tests/test_gpu_icp_edges.py): a point pairs with the live slot of the smallest distance, the
    lower slot on a tie; a NaN distance in a stream's first live slot rejects the point even when a later slot is finite
    (a NaN in a later slot is passed over); a neighbour index outside [0, n) rejects the point; a row of sums with a NaN in
    its gradient is refused like a bad pivot (bit 4, the pose untouched); a map cursor outside [0, map_size) is read as
    the nearest slot.
    ``graph=True``: ``register`` replays as one graph (the protocol of DESIGN.md section 21.2; ``calls``, ``captures``).
    ``register(..., trace=True)`` (``graph=False`` only) also returns, per iteration, clones of the queries, ``idx``,
    ``dist``, the summed row, ``delta`` and ``T``.

    One engine runs both modes: the graph (begin, stage, ``iters`` x (queries, search, accumulate, solve), push: ``4 + 4
    iters + 1`` launches) reads two (S,) words from device memory.  ``active[s]``: stream s delivered a frame in this call;
    ``restart[s]`` (looked at only where active): that frame starts a new sequence.  Per stream:
      idle (not active)     nothing of the stream changes (map slots, A, R, live, cursor); ``T[s]`` is ``init[s]`` bit for
                            bit, status ``IDLE`` (8), iterations = pairs = 0, cost = 0; its row of ``cloud`` is ignored
      restart               the map is emptied on the device, inside the graph, before the iterations; the frame finds no
                            live slot, freezes in iteration 0 with the few-pairs bit, returns ``init`` and fills slot 0
      pair (otherwise)      the registration and push, bit for bit those of a refiner of the stream's own
    The search and the staging run for every stream, so an idle stream costs what an active one does bar the gathers.
    ``reset()`` / ``reset(streams=...)`` arm a restart for the streams' next delivered frame, on the device and without a
    sync (``map_state()`` shows the old map until then).  Lock step is the view "all active, none restarting": its words
    are written once and no later call touches them.

    ``per_stream=True``: ``register(cloud, init, active=None, restart=None)`` takes the two masks, bool or integer, host
    sequences or device tensors (device tensors are copied on the device, without a sync); ``None`` = all active, none
    restarting.  The first call needs an active stream: the idle streams' rows of the persistent cloud start as copies of
    the first active stream's (the mask is read once, there), so that staging never sees data no caller supplied.
    ``trace=True`` returns ``(T, steps, masks)``.

    ``keyframe=dict(trans=0.1, rot=0.3)`` (metres, degrees): a frame goes into the map only when
    the motion accumulated since the stream's last inserted frame exceeds one of the thresholds (the reference's
    ``__update_map``); otherwise the map is only moved into the new frame.  One launch more per ``register``, between the
    last solve and the push, decides on the device; the graph's node sequence is the same for every decision.  A stream
    whose map is empty (first frame, restart, ``reset``) always inserts.  ``keyframe_state()`` shows the gate's words.
    ``None`` (the default) inserts every frame with the launches and bits of a refiner without the keyword.

    ``adopt_words(active, restart)``, before the first call: the graph reads the caller's two (S,) int32 0 / 1 device words
    instead (``StreamingOdometry``'s, which its step's graph has just written); ``register_adopted(cloud, init)`` then
    loads no mask at all."""

    _name = "IcpRefiner"        # in front of the messages of the methods a subclass shares
    _graph = property(lambda self: self.replay.graph())     # read-only: the captured graph or None, as the tests read it

    def __init__(self, streams, num_points, map_size=4, iters=10, sigma=0.5, max_dist=1.0, k_normals=10, damping=1e-6,
                 threshold_delta_pose=1e-4, min_pairs=64, graph=True, per_stream=False, keyframe=None):
        what, n, k = self._name, int(num_points), int(k_normals)
        self.keyframe = keyframe_args(what, keyframe)               # None or (trans, rot)
        self.streams = stream_count(what, streams, MAX_STREAMS)
        if not 64 <= n <= 16384:
            raise ValueError("%s: num_points=%d outside [64, 16384] (the neighbour search's range)" % (what, n))
        self._need_map(map_size)
        need_iters(what, iters)
        need_sigma(what, sigma)
        self._need_max_dist(max_dist)
        if not 1 <= k <= min(63, n - 1):
            raise ValueError("%s: k_normals=%d outside [1, %d]" % (what, k, min(63, n - 1)))
        need_solver(what, damping, threshold_delta_pose, min_pairs)
        self.num_points, self.iters, self.k_normals = n, int(iters), k
        self.sigma, self.max_dist, self.damping = float(sigma), float(max_dist), float(damping)
        self.threshold_delta_pose, self.min_pairs, self.graph = float(threshold_delta_pose), int(min_pairs), bool(graph)
        self.per_stream = bool(per_stream)
        self.bufs = None
        self.replay = Replay(graph)
        self._words = None          # adopt_words: the caller's (active, restart) words
        self._plain = False         # the refiner's own words are known to hold "all active, none restarting"

    def _need_map(self, map_size):
        """The map's own settings, checked where the constructor's order has them (a subclass has others)."""
        M = self.map_size = int(map_size)
        if not 1 <= M <= MAX_SLOTS or self.streams * M > 65535:
            raise ValueError("IcpRefiner: map_size=%d outside [1, %d] (and streams * map_size <= 65535)" % (M, MAX_SLOTS))

    def _need_max_dist(self, max_dist):
        need_max_dist(self._name, max_dist)

    # ---- state -------------------------------------------------------------------------------------------------------

    def _alloc(self, device):
        S, M, n, k = self.streams, self.map_size, self.num_points, self.k_normals
        lib = _lib.load()
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)
        f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=device)
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=device)
        eye = lambda *s: torch.eye(s[-1], dtype=torch.float64, device=device).expand(*s).contiguous()
        G = groups(n)
        assert G == lib.icp_accumulate_groups(n)
        self.bufs = dict(
            cloud=f32(S, n, 3), T=eye(S, 4, 4),
            stage_ws=torch.zeros((lib.knn_point_build_bytes(S, n),), dtype=torch.uint8, device=device),
            self_idx=i32(S, n, k + 1), stage_normals=f32(S, n, 3), stage_eig=f64(S, n, 3),
            map_xyz=f32(S, M, n, 3), map_normals=f32(S, M, n, 3),
            map_ws=torch.zeros((lib.knn_point_build_bytes(S * M, n),), dtype=torch.uint8, device=device),
            A=eye(S, M, 4, 4), R=eye(S, M, 3, 3), live=i32(S, M), cursor=i32(S),
            q=f32(S, M, n, 3), idx=i32(S, M, n), dist=f32(S, M, n), partial=f64(S, G, ROW),
            status=i32(S), iterations=i32(S), pairs=i32(S), cost=f64(S), sum=f64(S, ROW), delta=f64(S, 6),
            armed=i32(S))                    # restarts asked for by reset()
        active, restart = self._words or (i32(S), i32(S))
        self.bufs.update(active=active, restart=restart)            # the masks the graph reads
        if self.keyframe is not None:                               # the gate's words
            self.bufs.update(kf_delta=eye(S, 4, 4), kf_insert=i32(S), kf_count=i32(S))

    def _seed_structures(self):
        """Before the first registration: every slot's search structure becomes the first frame's (its live flag stays 0),
        so that no search ever walks memory that no build has written."""
        b, S, M = self.bufs, self.streams, self.map_size
        rows = b["stage_ws"].numel() // S // 33 * 32            # bytes per cloud: 64 * 16 of rows for every 32 of boxes
        boxes = rows // 32
        b["map_ws"][:S * M * rows].view(S, M, rows).copy_(b["stage_ws"][:S * rows].view(S, 1, rows).expand(S, M, rows))
        b["map_ws"][S * M * rows:].view(S, M, boxes).copy_(b["stage_ws"][S * rows:].view(S, 1, boxes).expand(S, M, boxes))

    def status(self):
        """(S,) int32 device view: 0 = the stream moved in every iteration of the last registration, else the bits of why
        it froze (1 converged, 2 too few pairs, 4 pivot not positive; masked registration: 8 idle, the stream delivered no
        frame in that call).  None before the first call."""
        return None if self.bufs is None else self.bufs["status"]

    def diagnostics(self):
        """Device views of the last registration: iterations used, pairs and the weighted cost sum w^2 r^2 of the last
        iteration a stream took part in (masked registration: all 0 for an idle stream; 1, 0, 0 for one that restarted).
        None before the first call."""
        if self.bufs is None:
            return None
        return dict(iterations=self.bufs["iterations"], pairs=self.bufs["pairs"], cost=self.bufs["cost"])

    def map_state(self):
        """Device views of the maps' bookkeeping: A (S, M, 4, 4) previous frame -> slot, R (S, M, 3, 3) slot -> previous
        frame, live (S, M), cursor (S,)."""
        if self.bufs is None:
            return None
        return {k: self.bufs[k] for k in ("A", "R", "live", "cursor")}

    def keyframe_state(self):
        """With ``keyframe=``: device views of the gate's words: delta (S, 4, 4) fp64 the motion since the stream's last
        inserted frame, insert (S,) int32 the last call's decision, count (S,) int32 the frames inserted since the map was
        emptied.  None before the first call or without ``keyframe``."""
        if self.bufs is None or self.keyframe is None:
            return None
        return dict(delta=self.bufs["kf_delta"], insert=self.bufs["kf_insert"], count=self.bufs["kf_count"])

    def reset(self, streams=None):
        """Empty the maps of all streams, or of ``streams`` (host stream indices, or an (S,) bool mask, host or device):
        their next delivered frame only fills the map.  The streams are armed on the device, without a sync, and the
        first launch of that frame's registration empties the map.  No new capture: the word is device memory that the
        graph reads."""
        mask = None if streams is None else stream_masks.stream_mask(streams, self.streams, "streams", self._name, True)
        if self.bufs is None:
            return
        armed = self.bufs["armed"]
        if mask is None:
            armed.fill_(1)
        else:
            armed.copy_(torch.maximum(armed, mask.to(armed.device)))

    # ---- one registration ----------------------------------------------------------------------------------------------

    def _stage(self):
        """The new frame's search structure, own neighbours and normals: what its slot will hold."""
        b, S, n, k = self.bufs, self.streams, self.num_points, self.k_normals
        dev = b["cloud"].device
        _lib.call("knn_build_kernel_wrapper", dev, S, n, _p(b["cloud"]), _p(b["stage_ws"]), 0)
        _lib.call("knn_point_prebuilt_kernel_wrapper", dev, S, n, n, k + 1, _p(b["cloud"]), _p(b["self_idx"]), 0,
                  _p(b["stage_ws"]))
        _lib.call("icp_normals_kernel_wrapper", dev, S, n, k, _p(b["cloud"]), _p(b["self_idx"]), _p(b["stage_normals"]),
                  _p(b["stage_eig"]))

    def _iterate(self, trace=None):
        b, S, M, n = self.bufs, self.streams, self.map_size, self.num_points
        dev = b["cloud"].device
        G = b["partial"].shape[1]
        active = _p(b["active"])
        for it in range(self.iters):
            _lib.call("icp_queries_masked_kernel_wrapper", dev, S, M, n, _p(b["A"]), _p(b["T"]), _p(b["cloud"]), _p(b["q"]),
                      active)
            _lib.call("knn_point_prebuilt_kernel_wrapper", dev, S * M, n, n, 1, _p(b["q"]), _p(b["idx"]), _p(b["dist"]),
                      _p(b["map_ws"]))
            _lib.call("icp_accumulate_masked_kernel_wrapper", dev, S, M, n, _p(b["cloud"]), _p(b["q"]), _p(b["idx"]),
                      _p(b["dist"]), _p(b["map_xyz"]), _p(b["map_normals"]), _p(b["live"]), _p(b["R"]), _p(b["T"]),
                      self.sigma, self.max_dist, _p(b["partial"]), active)
            if trace is not None:
                before = b["T"].clone()
            _lib.call("icp_solve_masked_kernel_wrapper", dev, S, G, it, _p(b["partial"]), self.damping,
                      self.threshold_delta_pose, self.min_pairs, _p(b["T"]), _p(b["status"]), _p(b["iterations"]),
                      _p(b["pairs"]), _p(b["cost"]), _p(b["sum"]), _p(b["delta"]), active)
            if trace is not None:
                trace.append(dict(q=b["q"].clone(), idx=b["idx"].clone(), dist=b["dist"].clone(), sum=b["sum"].clone(),
                                  delta=b["delta"].clone(), T_before=before, T=b["T"].clone(),
                                  status=b["status"].clone()))

    def _push(self):
        b, S, M, n = self.bufs, self.streams, self.map_size, self.num_points
        if self.keyframe is not None:                       # the gate, then the push that reads its decision
            dev = b["cloud"].device
            _lib.call("keyframe_gate_kernel_wrapper", dev, S, M, _p(b["T"]), _p(b["live"]), _p(b["active"]),
                      self.keyframe[0], self.keyframe[1], _p(b["kf_delta"]), _p(b["kf_insert"]), _p(b["kf_count"]))
            _lib.call("keyframe_icp_push_kernel_wrapper", dev, S, M, n, _p(b["T"]), _p(b["cloud"]), _p(b["stage_normals"]),
                      _p(b["stage_ws"]), _p(b["map_xyz"]), _p(b["map_normals"]), _p(b["map_ws"]), _p(b["A"]), _p(b["R"]),
                      _p(b["live"]), _p(b["cursor"]), _p(b["active"]), _p(b["kf_insert"]))
            return
        _lib.call("icp_map_push_masked_kernel_wrapper", b["cloud"].device, S, M, n, _p(b["T"]), _p(b["cloud"]),
                  _p(b["stage_normals"]), _p(b["stage_ws"]), _p(b["map_xyz"]), _p(b["map_normals"]), _p(b["map_ws"]),
                  _p(b["A"]), _p(b["R"]), _p(b["live"]), _p(b["cursor"]), _p(b["active"]))

    def _begin(self):
        """Empty the maps of the streams whose frame starts a new sequence (``restart``, or armed by ``reset``)."""
        b = self.bufs
        _lib.call("icp_begin_kernel_wrapper", b["cloud"].device, self.streams, self.map_size, _p(b["active"]),
                  _p(b["restart"]), _p(b["armed"]), _p(b["A"]), _p(b["R"]), _p(b["live"]), _p(b["cursor"]))

    def _body(self, trace=None):
        self._begin()
        self._stage()
        self._iterate(trace)
        self._push()

    def _check(self, cloud, init):
        S, n = self.streams, self.num_points
        if not isinstance(cloud, torch.Tensor) or cloud.dtype != torch.float32 or tuple(cloud.shape) != (S, n, 3):
            raise ValueError("%s: cloud must be float32 (%d, %d, 3), got %s %s"
                             % (self._name, S, n, getattr(cloud, "dtype", type(cloud)), tuple(getattr(cloud, "shape", ()))))
        init_poses(self._name, init, S)
        need_cuda(cloud, init)

    def _mask(self, mask, what):
        return stream_masks.stream_mask(mask, self.streams, what, self._name)

    def adopt_words(self, active, restart):
        """Before the first call: the graph reads the caller's (S,) int32 0 / 1 device words, which the caller writes
        before every ``register_adopted`` (a lock-step view's ``active`` holds ones)."""
        if self.bufs is not None:
            raise RuntimeError("%s: adopt_words comes before the first call (a captured graph keeps its words)" % self._name)
        _need_mask(active, self._name, self.streams)
        _need(restart, "%s: restart" % self._name, torch.int32, (self.streams,))
        self._words = (active, restart)

    def register_adopted(self, cloud, init, all_active=False):
        """``register`` with this call's masks already in the adopted words: no mask is parsed, copied or loaded.
        ``all_active``: the caller knows on the host that ``active`` holds ones (the cloud then goes in as a plain copy)."""
        if self._words is None:
            raise RuntimeError("%s: register_adopted needs adopt_words(active, restart)" % self._name)
        return self._register(cloud, init, every=bool(all_active))

    def register(self, cloud, init, active=None, restart=None, trace=False):
        if trace and self.graph:
            raise ValueError("%s: trace=True needs graph=False (a replayed graph cannot hand out its iterations)" % self._name)
        if not self.per_stream and (active is not None or restart is not None):
            raise ValueError("%s: active / restart masks need per_stream=True" % self._name)
        if self._words is not None:
            raise RuntimeError("%s: the words are the caller's (adopt_words): call register_adopted" % self._name)
        act = None if active is None else self._mask(active, "active")
        rst = None if restart is None else self._mask(restart, "restart")
        return self._register(cloud, init, act, rst, trace, every=act is None)

    def _register(self, cloud, init, act=None, rst=None, trace=False, every=False):
        from . import fused
        self._check(cloud, init)
        first, own, plain = self.bufs is None, self._words is None, act is None and rst is None
        if first:                                           # every row of the cloud starts defined; the per-stream view
            seen = None if not self.per_stream else act if own else self._words[0]        # reads the mask once, here
            _, cloud = stream_masks.seed_idle_rows(seen, self.streams, self._name, cloud)
        if init.dim() == 2:
            init = evaluation.rows_to_transforms(init)
        if first:
            self._alloc(cloud.device)
        b = self.bufs
        if own and not (plain and self._plain):             # words that hold "all active, none restarting" are left alone
            stream_masks.load_words(b["active"], b["restart"], act, rst)
            self._plain = plain
        if first or every:                                  # every: all streams are active, as the host knows
            b["cloud"].copy_(cloud)
        else:                                               # the active streams' rows only, one launch
            src = cloud.contiguous()
            fused.masked_copy([(b["cloud"].data_ptr(), src.data_ptr(), self.num_points * 12)], b["active"])
        b["T"].copy_(init)
        if first:
            self._stage()
            self._seed_structures()
        steps = [] if trace else None
        self.replay.run(lambda: self._body(steps), cloud.device)
        if trace and self.per_stream:
            return b["T"], steps, dict(active=b["active"].clone(), restart=b["restart"].clone())
        return (b["T"], steps) if trace else b["T"]
