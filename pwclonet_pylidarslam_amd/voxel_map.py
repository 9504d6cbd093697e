"""Point-to-plane registration of incoming frames against a persistent voxel map per stream.

``registration.IcpRefiner`` forgets a frame after ``map_size`` pushes and searches every slot in every iteration.
``VoxelMapRefiner`` keeps one local map per stream for as long as the sensor stays near it: a toroidal grid of ``extent``
voxels of edge ``voxel_size``, eight points (one per octant) and their normals per voxel, in the stream's map frame (the
frame of the first registered frame).  A lookup is a fixed gather of 27 voxels, so an iteration is two launches
(accumulate, solve) whatever the number of frames in the map:

    ref = VoxelMapRefiner(streams=S, num_points=8192)
    T = ref.register(cloud, init)          # as IcpRefiner.register: T maps the frame into the previous frame

The kernels are ``csrc/voxel_map.hip``; the staging (search structure, self-search, normals) and the solver are the knn
refiner's, unchanged.  There is no CPU path.
"""
import numpy as np
import torch

from . import _lib, registration
from .registration import ROW, _need, _need_mask, _p, groups
from .stream_engine import need_sigma, stream_index

MAX_STREAMS = 1024                               # csrc/voxel_map.hpp: VM_MAX_STREAMS, VM_MAX_AXIS, VM_CELL_BYTES
MAX_AXIS = 1024
CELL_BYTES = 264
EMPTY = -1                                       # an empty coordinate word or key, read as int64
BIAS = 1 << 20


def extent_args(what, voxel_size, extent):
    """-> (voxel_size, (Nx, Ny, Nz)); ValueError naming the argument otherwise."""
    ok = isinstance(voxel_size, (int, float, np.integer, np.floating)) and not isinstance(voxel_size, bool)
    if not ok or not np.isfinite(float(voxel_size)) or not float(voxel_size) > 0.0:
        raise ValueError("%s: voxel_size=%r must be finite and > 0" % (what, voxel_size))
    try:
        ext = tuple(int(v) for v in extent)
        whole = all(float(v) == int(v) for v in extent)
    except (TypeError, ValueError):
        ext, whole = (), False
    if len(ext) != 3 or not whole or any(v < 4 or v > MAX_AXIS or v % 2 for v in ext) or ext[0] * ext[1] * ext[2] >= 1 << 28:
        raise ValueError("%s: extent=%r must be three even voxel counts in [4, %d] with Nx Ny Nz < 2^28"
                         % (what, extent, MAX_AXIS))
    return float(voxel_size), ext


def map_bytes(S, extent):
    """Bytes of the grid buffer of S streams: 264 per voxel."""
    return int(S) * extent[0] * extent[1] * extent[2] * CELL_BYTES


def new_grid(S, extent, device):
    """An empty grid buffer of S streams: every coordinate word and key all ones, points and normals zero."""
    cells = extent[0] * extent[1] * extent[2]
    assert _lib.load().voxel_map_bytes(S, *extent) == map_bytes(S, extent)
    grid = torch.zeros((map_bytes(S, extent),), dtype=torch.uint8, device=device)
    grid[:S * cells * 72] = 255
    return grid


def sections(grid, S, extent):
    """Views of a grid buffer: coord (S, cells) int64, keys (S, cells, 8) int64 (-1: empty), points and normals (S, cells,
    8, 3) fp32."""
    cells = extent[0] * extent[1] * extent[2]
    a, b, c = S * cells * 8, S * cells * 72, S * cells * 168
    return dict(coord=grid[:a].view(torch.int64).view(S, cells), keys=grid[a:b].view(torch.int64).view(S, cells, 8),
                points=grid[b:c].view(torch.float32).view(S, cells, 8, 3),
                normals=grid[c:].view(torch.float32).view(S, cells, 8, 3))


def _need_grid(what, grid, S, extent):
    _need(grid, "%s: grid" % what, torch.uint8, (map_bytes(S, extent),))


def _need_state(what, S, P, nonempty, seq):
    _need(P, "%s: P" % what, torch.float64, (S, 4, 4))
    _need(nonempty, "%s: nonempty" % what, torch.int32, (S, 1))
    _need(seq, "%s: seq" % what, torch.int32, (S,))


def _streams(what, t, name):
    if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[-1] != 3:
        raise ValueError("%s: %s must be (S, n, 3), got %s" % (what, name, tuple(getattr(t, "shape", ()))))
    if not 1 <= t.shape[0] <= MAX_STREAMS:
        raise ValueError("%s: S=%d outside [1, %d]" % (what, t.shape[0], MAX_STREAMS))
    return t.shape[0], t.shape[1]


# ---- the ops alone -----------------------------------------------------------------------------------------------------

def begin(grid, extent, P, nonempty, seq, active=None, restart=None, armed=None):
    """First launch of a registration, in place: the streams with ``active and (restart or armed)`` (masks (S,) int32;
    ``active=None``: all, the others: none) get an empty map: coordinate words all ones, P = I, nonempty = 0, seq = 0.
    ``armed`` is only read: ``pose`` clears it."""
    S = P.shape[0] if isinstance(P, torch.Tensor) and P.dim() == 3 else 0
    _, extent = extent_args("begin", 1.0, extent)
    _need_state("begin", S, P, nonempty, seq)
    _need_grid("begin", grid, S, extent)
    for name, m in (("active", active), ("restart", restart), ("armed", armed)):
        if m is not None:
            _need(m, "begin: %s" % name, torch.int32, (S,))
    _lib.call("voxel_begin_kernel_wrapper", grid.device, S, *extent, _p(active), _p(restart), _p(armed), _p(grid), _p(P),
              _p(nonempty), _p(seq))


def insert(grid, extent, voxel_size, cloud, normals, P, seq, T=None, nonempty=None, active=None, insert=None, slot=None):
    """Inserts cloud / normals (S, n, 3) fp32 into the grid with the pose P (S, 4, 4) fp64, or P T where T is given, or the
    identity for the streams whose ``nonempty`` (S, 1) word is given and zero; keys carry ``seq`` (S,) int32.  ``active`` /
    ``insert`` (S,) int32 or None: only the streams with both set insert.  -> slot (S, n) int32: cell * 8 + octant every row
    asked for, -1 where it was not inserted.  Three launches; P, nonempty and seq are ``pose``'s to move on."""
    S, n = _streams("insert", cloud, "cloud")
    voxel_size, extent = extent_args("insert", voxel_size, extent)
    _need(cloud, "insert: cloud", torch.float32, (S, n, 3))
    _need(normals, "insert: normals", torch.float32, (S, n, 3))
    _need(P, "insert: P", torch.float64, (S, 4, 4))
    _need(seq, "insert: seq", torch.int32, (S,))
    _need_grid("insert", grid, S, extent)
    if T is not None:
        _need(T, "insert: T", torch.float64, (S, 4, 4))
    if nonempty is not None:
        _need(nonempty, "insert: nonempty", torch.int32, (S, 1))
    for name, m in (("active", active), ("insert", insert)):
        if m is not None:
            _need(m, "insert: %s" % name, torch.int32, (S,))
    if slot is None:
        slot = torch.full((S, n), -1, dtype=torch.int32, device=cloud.device)
    _need(slot, "insert: slot", torch.int32, (S, n))
    _lib.call("voxel_insert_kernel_wrapper", cloud.device, S, n, *extent, voxel_size, _p(cloud), _p(normals), _p(P), _p(T),
              _p(nonempty), _p(seq), _p(grid), _p(slot), _p(active), _p(insert))
    return slot


def pose(P, nonempty, seq, T=None, armed=None, active=None, insert=None):
    """After ``insert``, in place: P = I where nonempty was zero, else P T (``T=None``: P stays); the streams that inserted
    get seq += 1 and nonempty = 1; ``armed`` is cleared for the active streams."""
    S = P.shape[0] if isinstance(P, torch.Tensor) and P.dim() == 3 else 0
    if not 1 <= S <= MAX_STREAMS:
        raise ValueError("pose: S=%d outside [1, %d]" % (S, MAX_STREAMS))
    _need_state("pose", S, P, nonempty, seq)
    if T is not None:
        _need(T, "pose: T", torch.float64, (S, 4, 4))
    for name, m in (("armed", armed), ("active", active), ("insert", insert)):
        if m is not None:
            _need(m, "pose: %s" % name, torch.int32, (S,))
    _lib.call("voxel_pose_kernel_wrapper", P.device, S, _p(T), _p(P), _p(nonempty), _p(seq), _p(armed), _p(active),
              _p(insert))


def accumulate(grid, extent, voxel_size, p, P, T=None, sigma=0.5, max_dist=1.0, active=None, nearest=False):
    """One launch of the hot path -> partial (S, groups(n), 32) fp64 in ``registration.solve``'s layout.  p (S, n, 3) fp32; P
    (S, 4, 4) fp64 the pose of the previous frame in the map frame; T (S, 4, 4) fp64 the frame's pose estimate (None: the
    identity).  ``nearest=True`` -> (partial, cell, octant, dist): per point the nearest stored point among the 27 voxels
    around fp32(P T p), (S, n) int32, int32 and fp32; -1, -1 and +Inf where there is none."""
    S, n = _streams("accumulate", p, "p")
    voxel_size, extent = extent_args("accumulate", voxel_size, extent)
    need_sigma("accumulate", sigma)
    if not 0.0 <= float(max_dist) <= voxel_size:
        raise ValueError("accumulate: max_dist=%r outside [0, voxel_size=%r] (the 27 voxels hold every point that near)"
                         % (max_dist, voxel_size))
    _need(p, "accumulate: p", torch.float32, (S, n, 3))
    _need(P, "accumulate: P", torch.float64, (S, 4, 4))
    if T is not None:
        _need(T, "accumulate: T", torch.float64, (S, 4, 4))
    if active is not None:
        _need_mask(active, "accumulate", S)
    _need_grid("accumulate", grid, S, extent)
    dev = p.device
    partial = torch.empty((S, groups(n), ROW), dtype=torch.float64, device=dev)
    cell = octant = dist = None
    if nearest:                                      # an idle stream's rows are not written, so they start defined
        cell = torch.full((S, n), -1, dtype=torch.int32, device=dev)
        octant = torch.full((S, n), -1, dtype=torch.int32, device=dev)
        dist = torch.full((S, n), float("inf"), dtype=torch.float32, device=dev)
    _lib.call("voxel_accumulate_kernel_wrapper", dev, S, n, *extent, voxel_size, _p(p), _p(P), _p(T), _p(grid), float(sigma),
              float(max_dist), _p(partial), _p(cell), _p(octant), _p(dist), _p(active))
    return (partial, cell, octant, dist) if nearest else partial


def nearest(grid, extent, voxel_size, p, P, T=None, active=None):
    """-> (cell, octant, dist) (S, n): the nearest stored point of every fp32(P T p), as ``accumulate(..., nearest=True)``
    finds it (no distance bound: that is the pair's)."""
    voxel_size, _ = extent_args("nearest", voxel_size, extent)
    return accumulate(grid, extent, voxel_size, p, P, T, max_dist=voxel_size, active=active, nearest=True)[1:]


def unpack(coord):
    """Coordinate words (int64 tensor or array, no empty word among them) -> (..., 3) voxel coordinates (cx, cy, cz)."""
    c = coord.cpu().numpy() if isinstance(coord, torch.Tensor) else np.asarray(coord)
    return np.stack([(c & 0x1FFFFF) - BIAS, ((c >> 21) & 0x1FFFFF) - BIAS, ((c >> 42) & 0x1FFFFF) - BIAS], axis=-1)


# ---- the refiner -------------------------------------------------------------------------------------------------------

class VoxelMapRefiner(registration.IcpRefiner):
    """Registers one frame per call and stream against the stream's persistent voxel map.

    ``register(cloud, init, active=None, restart=None, trace=False)``, ``adopt_words``, ``register_adopted``, ``status``,
    ``diagnostics``, ``reset(streams=None)`` and ``keyframe_state`` are ``registration.IcpRefiner``'s, with its semantics:
    the first frame after a reset only fills the map and returns ``init`` bit for bit (the map is empty, so the stream
    freezes in iteration 0 with the few-pairs bit); idle streams keep every bit of their grid, ``pose()`` and counters and
    get status ``IDLE``; a restart empties the map on the device, inside the graph.  One registration is ``1 + 3 + 2 iters
    + 4`` launches (begin; stage; accumulate and solve per iteration; three launches of insertion and the pose), one more
    with ``keyframe=``, and replays as one graph.

    The map: ``extent`` voxels (even, at least 4 per axis) of edge ``voxel_size`` around the sensor, 264 bytes each.  A
    frame is inserted with its absolute pose in the map frame; only points within ``(N / 2 - 1) voxel_size`` of the sensor
    on every axis go in, the first point ever to reach an octant stays, and a cell is taken over (its eight entries
    emptied) when a voxel one torus period away needs it.  ``max_dist <= voxel_size``, so that the 27 voxels around a
    query hold every stored point that near and the pair is the exact nearest stored point.  ``keyframe=dict(trans, rot)``
    gates the insertion as for the knn refiner; a frame that is not inserted still moves ``pose()``.

    ``pose()``: (S, 4, 4) fp64 device view, the pose of the last registered frame in the map frame.  ``map_points(stream)``:
    the stored entries, compacted.  ``map_bytes()``: bytes of the grid."""

    _name = "VoxelMapRefiner"

    def __init__(self, streams, num_points, voxel_size=1.0, extent=(128, 128, 32), iters=10, sigma=0.5, max_dist=1.0,
                 k_normals=10, damping=1e-6, threshold_delta_pose=1e-4, min_pairs=64, graph=True, per_stream=False,
                 keyframe=None):
        self.voxel_size, self.extent = voxel_size, extent            # checked by _need_map, where the parent's order has it
        super().__init__(streams, num_points, None, iters, sigma, max_dist, k_normals, damping, threshold_delta_pose,
                         min_pairs, graph, per_stream, keyframe)

    def _need_map(self, map_size):
        self.voxel_size, self.extent = extent_args(self._name, self.voxel_size, self.extent)

    def _need_max_dist(self, max_dist):
        if not 0.0 <= float(max_dist) <= self.voxel_size:
            raise ValueError("%s: max_dist=%r outside [0, voxel_size=%r]: the lookup reads the 27 voxels around a query, "
                             "which hold every stored point within one voxel edge" % (self._name, max_dist, self.voxel_size))

    # ---- state -------------------------------------------------------------------------------------------------------

    def _alloc(self, device):
        S, n, k = self.streams, self.num_points, self.k_normals
        lib = _lib.load()
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)
        f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=device)
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=device)
        eye = lambda *s: torch.eye(s[-1], dtype=torch.float64, device=device).expand(*s).contiguous()
        self.bufs = dict(
            cloud=f32(S, n, 3), T=eye(S, 4, 4),
            stage_ws=torch.zeros((lib.knn_point_build_bytes(S, n),), dtype=torch.uint8, device=device),
            self_idx=i32(S, n, k + 1), stage_normals=f32(S, n, 3), stage_eig=f64(S, n, 3),
            grid=new_grid(S, self.extent, device), P=eye(S, 4, 4), nonempty=i32(S, 1), seq=i32(S),
            slot=torch.full((S, n), -1, dtype=torch.int32, device=device), partial=f64(S, groups(n), ROW),
            status=i32(S), iterations=i32(S), pairs=i32(S), cost=f64(S), sum=f64(S, ROW), delta=f64(S, 6), armed=i32(S))
        active, restart = self._words or (i32(S), i32(S))
        self.bufs.update(active=active, restart=restart)
        if self.keyframe is not None:
            self.bufs.update(kf_delta=eye(S, 4, 4), kf_insert=i32(S), kf_count=i32(S))

    def _seed_structures(self):
        """Nothing to seed: the map has no search structure."""

    def map_state(self):
        """Device views of the map's bookkeeping: P (S, 4, 4), nonempty (S, 1), seq (S,)."""
        if self.bufs is None:
            return None
        return {k: self.bufs[k] for k in ("P", "nonempty", "seq")}

    def pose(self):
        """(S, 4, 4) fp64 device view: the pose of every stream's last registered frame in its map frame; None before the
        first call."""
        return None if self.bufs is None else self.bufs["P"]

    def map_bytes(self):
        return map_bytes(self.streams, self.extent)

    def map_points(self, stream):
        """The stored entries of one stream's map, compacted with torch ops (outside any graph; this syncs): dict(points
        (m, 3) fp32, normals (m, 3) fp32, voxels (m, 3) int64, octants (m,) int64, keys (m,) int64 = seq << 32 | row), in
        cell and octant order.  An entry counts where its cell has an owner and its key is not empty."""
        i = stream_index(self._name, None, stream, self.streams)
        if self.bufs is None:
            return None
        sec = sections(self.bufs["grid"], self.streams, self.extent)
        keep = (sec["coord"][i] != EMPTY)[:, None] & (sec["keys"][i] != EMPTY)
        cell, octant = keep.nonzero(as_tuple=True)
        voxels = torch.from_numpy(unpack(sec["coord"][i][cell])).reshape(-1, 3)
        return dict(points=sec["points"][i][cell, octant], normals=sec["normals"][i][cell, octant], voxels=voxels,
                    octants=octant, keys=sec["keys"][i][cell, octant])

    # ---- one registration ----------------------------------------------------------------------------------------------

    def _begin(self):
        b = self.bufs
        _lib.call("voxel_begin_kernel_wrapper", b["cloud"].device, self.streams, *self.extent, _p(b["active"]),
                  _p(b["restart"]), _p(b["armed"]), _p(b["grid"]), _p(b["P"]), _p(b["nonempty"]), _p(b["seq"]))

    def _iterate(self, trace=None):
        b, S, n = self.bufs, self.streams, self.num_points
        dev = b["cloud"].device
        G = b["partial"].shape[1]
        active = _p(b["active"])
        for it in range(self.iters):
            near = [None] * 3
            if trace is not None:
                near = [torch.full((S, n), -1, dtype=torch.int32, device=dev), torch.full((S, n), -1, dtype=torch.int32,
                        device=dev), torch.full((S, n), float("inf"), dtype=torch.float32, device=dev)]
            _lib.call("voxel_accumulate_kernel_wrapper", dev, S, n, *self.extent, self.voxel_size, _p(b["cloud"]), _p(b["P"]),
                      _p(b["T"]), _p(b["grid"]), self.sigma, self.max_dist, _p(b["partial"]), _p(near[0]), _p(near[1]),
                      _p(near[2]), active)
            if trace is not None:
                before = b["T"].clone()
            _lib.call("icp_solve_masked_kernel_wrapper", dev, S, G, it, _p(b["partial"]), self.damping,
                      self.threshold_delta_pose, self.min_pairs, _p(b["T"]), _p(b["status"]), _p(b["iterations"]),
                      _p(b["pairs"]), _p(b["cost"]), _p(b["sum"]), _p(b["delta"]), active)
            if trace is not None:
                trace.append(dict(cell=near[0], octant=near[1], dist=near[2], sum=b["sum"].clone(), delta=b["delta"].clone(),
                                  T_before=before, T=b["T"].clone(), status=b["status"].clone()))

    def _push(self):
        b, S, n = self.bufs, self.streams, self.num_points
        dev = b["cloud"].device
        ins = None
        if self.keyframe is not None:                       # the gate's "no live slot" is "the map is empty"
            _lib.call("keyframe_gate_kernel_wrapper", dev, S, 1, _p(b["T"]), _p(b["nonempty"]), _p(b["active"]),
                      self.keyframe[0], self.keyframe[1], _p(b["kf_delta"]), _p(b["kf_insert"]), _p(b["kf_count"]))
            ins = b["kf_insert"]
        _lib.call("voxel_insert_kernel_wrapper", dev, S, n, *self.extent, self.voxel_size, _p(b["cloud"]),
                  _p(b["stage_normals"]), _p(b["P"]), _p(b["T"]), _p(b["nonempty"]), _p(b["seq"]), _p(b["grid"]),
                  _p(b["slot"]), _p(b["active"]), _p(ins))
        _lib.call("voxel_pose_kernel_wrapper", dev, S, _p(b["T"]), _p(b["P"]), _p(b["nonempty"]), _p(b["seq"]),
                  _p(b["armed"]), _p(b["active"]), _p(ins))
