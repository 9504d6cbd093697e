"""Projective frame-to-model registration on spherical vertex maps, on the device.

The reference's default odometry is ``ICPFrameToModel`` over a ``ProjectiveLocalMap`` (R/slam/odometry/local_map.py:84-240,
R = /root/reference): every sweep becomes a spherical vertex map (R/slam/common/projection.py:20-82, 340-436), normals come
from box-filtered moments of that image (R/slam/common/geometry.py:248-303), the last frames are re-projected into the
newest frame's view and a point's neighbour is whatever sits at its own pixel (geometry.py:405-447): no search structure,
and every point of the sweep takes part.  ``ProjectiveIcpRefiner`` does that with the kernels of ``csrc/projective.hip`` and
the solver of ``registration`` (section 21):

    ref = ProjectiveIcpRefiner(streams=S, capacity=131072, height=64, width=1800)
    T = ref.register(points, lengths, init)     # points (S, capacity, 3|4) fp32, lengths (S,), init (S, 4, 4) fp64 or (S, 7)

``T`` maps the frame's points into the previous frame, as ``registration.IcpRefiner``'s does.  There is no CPU path.
"""
import numpy as np
import torch

from . import _lib, evaluation, registration
from .registration import _need, _p, BAD_PIVOT, CONVERGED, FEW_PAIRS, ROW    # noqa: F401  (the status bits are section 21's)
from .stream_engine import (Replay, Replayed, init_poses, need_cuda, need_iters, need_max_dist, need_sigma, need_solver,
                            stream_count)

MAX_STREAMS = registration.MAX_STREAMS
MAX_SLOTS = registration.MAX_SLOTS
KERNEL_SIZES = (3, 5)                            # csrc/projective.hip: the instantiated windows


def _image_args(what, height, width, up_fov, down_fov):
    H, W, up, down = int(height), int(width), float(up_fov), float(down_fov)
    if H < 1 or W < 1 or H * W * 3 >= 1 << 31:
        raise ValueError("%s: height=%d, width=%d out of range" % (what, H, W))
    if not (np.isfinite(up) and np.isfinite(down)) or abs(up) + abs(down) <= 0.0:
        raise ValueError("%s: up_fov=%r, down_fov=%r must be finite and span an angle" % (what, up_fov, down_fov))
    return H, W, up, down


# ---- the ops alone -----------------------------------------------------------------------------------------------------

def vertex_map(points, lengths=None, keep=None, height=64, width=1800, up_fov=3.0, down_fov=-24.8, workspace=None):
    """points (S, R, 3|4) fp32; ``lengths`` (S,) int32 on the device: stream s offers rows ``[:lengths[s]]``; ``keep`` (S, R)
    int32: only rows with keep != 0 (both as ``preprocess.compact`` / ``deskew`` pass them; at least one is required, both
    may be given) -> (vmap (S, H, W, 3) fp32: per pixel the nearest point, the lowest row among equal ranges, zero where
    empty; rows (S, H, W) int32: that point's row, -1 where empty)."""
    what = "vertex_map"
    H, W, up, down = _image_args(what, height, width, up_fov, down_fov)
    if not isinstance(points, torch.Tensor) or points.dim() != 3 or points.shape[-1] not in (3, 4):
        raise ValueError("%s: points must be (S, R, 3|4), got %s" % (what, tuple(getattr(points, "shape", ()))))
    S, R, C = points.shape
    if lengths is None and keep is None:
        raise ValueError("%s: lengths (S,) or a keep mask (S, R) is required" % what)
    if S < 1 or R < 1 or S > 65535:
        raise ValueError("%s: S=%d, R=%d out of range" % (what, S, R))
    _need(points, "%s: points" % what, torch.float32)
    if lengths is not None:
        _need(lengths, "%s: lengths" % what, torch.int32, (S,))
    if keep is not None:
        _need(keep, "%s: keep" % what, torch.int32, (S, R))
    dev = points.device
    if workspace is None:
        workspace = torch.empty((_lib.load().proj_vertex_map_workspace_bytes(S, H, W),), dtype=torch.uint8, device=dev)
    vmap = torch.empty((S, H, W, 3), dtype=torch.float32, device=dev)
    rows = torch.empty((S, H, W), dtype=torch.int32, device=dev)
    _lib.call("proj_vertex_map_kernel_wrapper", dev, S, R, C, H, W, up, down, _p(points), _p(lengths), _p(keep),
              _p(workspace), _p(vmap), _p(rows))
    return vmap, rows


def normal_map(vmap, kernel_size=5):
    """vmap (B, H, W, 3) fp32 -> normals (B, H, W, 3) fp32 as the reference's ``compute_normal_map``: n = C^-1 m from the
    window's moments about the sensor (fp64 sums, one rounding), unit length, pointing away from the sensor; zero where
    |det C| <= 1e-6, where n vanishes or where the centre pixel is empty."""
    if not isinstance(vmap, torch.Tensor) or vmap.dim() != 4 or vmap.shape[-1] != 3:
        raise ValueError("normal_map: vmap must be (B, H, W, 3), got %s" % (tuple(getattr(vmap, "shape", ())),))
    if int(kernel_size) not in KERNEL_SIZES:
        raise ValueError("normal_map: kernel_size=%r is not instantiated (%s)" % (kernel_size, " or ".join(map(str, KERNEL_SIZES))))
    B, H, W, _ = vmap.shape
    if B < 1 or B > 65535 or H < 1 or W < 1:
        raise ValueError("normal_map: B=%d H=%d W=%d out of range" % (B, H, W))
    _need(vmap, "normal_map: vmap", torch.float32)
    out = torch.empty_like(vmap)
    _lib.call("proj_normal_map_kernel_wrapper", vmap.device, B, H, W, int(kernel_size), _p(vmap), _p(out))
    return out


def model_build(map_v, map_n, A, live, up_fov=3.0, down_fov=-24.8, workspace=None):
    """map_v / map_n (S, M, H, W, 3) fp32: every slot's images in the slot's own frame; A (S, M, 4, 4) fp64: the newest
    frame -> slot; live (S, M) int32 -> (model_v, model_n (S, M, H, W, 3): every live slot re-projected into the newest
    frame's view, one image per slot (the reference's ``build_model``); src (S, M, H, W) int32: the slot's pixel index that
    won, -1 where empty).  A slot that is not live gives an empty image."""
    if not isinstance(map_v, torch.Tensor) or map_v.dim() != 5 or map_v.shape[-1] != 3:
        raise ValueError("model_build: map_v must be (S, M, H, W, 3)")
    S, M, H, W, _ = map_v.shape
    H, W, up, down = _image_args("model_build", H, W, up_fov, down_fov)
    if not 1 <= M <= MAX_SLOTS or S < 1 or S * M > 65535:
        raise ValueError("model_build: S=%d M=%d out of range (M <= %d, S * M <= 65535)" % (S, M, MAX_SLOTS))
    _need(map_v, "model_build: map_v", torch.float32)
    _need(map_n, "model_build: map_n", torch.float32, (S, M, H, W, 3))
    _need(A, "model_build: A", torch.float64, (S, M, 4, 4))
    _need(live, "model_build: live", torch.int32, (S, M))
    dev = map_v.device
    if workspace is None:
        workspace = torch.empty((_lib.load().proj_model_build_workspace_bytes(S, M, H, W),), dtype=torch.uint8, device=dev)
    model_v, model_n = torch.empty_like(map_v), torch.empty_like(map_v)
    src = torch.empty((S, M, H, W), dtype=torch.int32, device=dev)
    _lib.call("proj_model_build_kernel_wrapper", dev, S, M, H, W, up, down, _p(map_v), _p(map_n), _p(A), _p(live),
              _p(workspace), _p(model_v), _p(model_n), _p(src))
    return model_v, model_n, src


def accumulate(vmap, model_v, model_n, T, up_fov=3.0, down_fov=-24.8, sigma=0.5, max_dist=1.0, with_pairs=False):
    """One launch of the normal equations' sums over projective pairs -> partial (S, groups(H * W), 32) fp64 in
    ``registration.solve``'s layout.  vmap (S, H, W, 3): the new frame's own vertex map; model_v / model_n (S, M, H, W, 3);
    T (S, 4, 4) fp64.  ``with_pairs``: also (slot, pixel) (S, H, W) int32: the chosen slot (-1: no pair) and the pixel
    index of the moved point (-1: none)."""
    if not isinstance(model_v, torch.Tensor) or model_v.dim() != 5 or model_v.shape[-1] != 3:
        raise ValueError("accumulate: model_v must be (S, M, H, W, 3)")
    S, M, H, W, _ = model_v.shape
    H, W, up, down = _image_args("accumulate", H, W, up_fov, down_fov)
    registration._need_pairing(sigma, max_dist)
    if not 1 <= M <= MAX_SLOTS or S < 1 or S > 65535:
        raise ValueError("accumulate: S=%d M=%d out of range (M <= %d)" % (S, M, MAX_SLOTS))
    _need(vmap, "accumulate: vmap", torch.float32, (S, H, W, 3))
    _need(model_v, "accumulate: model_v", torch.float32)
    _need(model_n, "accumulate: model_n", torch.float32, (S, M, H, W, 3))
    _need(T, "accumulate: T", torch.float64, (S, 4, 4))
    dev = vmap.device
    partial = torch.empty((S, registration.groups(H * W), ROW), dtype=torch.float64, device=dev)
    slot = pixel = None
    if with_pairs:
        slot = torch.empty((S, H, W), dtype=torch.int32, device=dev)
        pixel = torch.empty((S, H, W), dtype=torch.int32, device=dev)
    _lib.call("proj_accumulate_kernel_wrapper", dev, S, M, H, W, up, down, _p(vmap), _p(model_v), _p(model_n), _p(T),
              float(sigma), float(max_dist), _p(partial), _p(slot), _p(pixel))
    return (partial, slot, pixel) if with_pairs else partial


def map_push(T, vmap, nmap, map_v, map_n, A, live, cursor):
    """The handover after a registration, in place: vmap / nmap (S, H, W, 3) go into slot cursor[s] of map_v / map_n
    (S, M, H, W, 3), the other live slots get A <- A T, the new slot A = I and live = 1, the cursor moves on."""
    if not isinstance(map_v, torch.Tensor) or map_v.dim() != 5:
        raise ValueError("map_push: map_v must be (S, M, H, W, 3)")
    S, M, H, W, _ = map_v.shape
    _need(T, "map_push: T", torch.float64, (S, 4, 4))
    _need(vmap, "map_push: vmap", torch.float32, (S, H, W, 3))
    _need(nmap, "map_push: nmap", torch.float32, (S, H, W, 3))
    _need(map_v, "map_push: map_v", torch.float32, (S, M, H, W, 3))
    _need(map_n, "map_push: map_n", torch.float32, (S, M, H, W, 3))
    _need(A, "map_push: A", torch.float64, (S, M, 4, 4))
    _need(live, "map_push: live", torch.int32, (S, M))
    _need(cursor, "map_push: cursor", torch.int32, (S,))
    _lib.call("proj_map_push_kernel_wrapper", T.device, S, M, H, W, _p(T), _p(vmap), _p(nmap), _p(map_v), _p(map_n), _p(A),
              _p(live), _p(cursor))


# ---- the refiner -------------------------------------------------------------------------------------------------------

class ProjectiveIcpRefiner(Replayed):
    """Registers one sweep per call and stream against each stream's map of the last ``map_size`` frames' vertex maps.

    ``register(points, lengths, init)``: points (S, R <= capacity, 3|4) fp32 (the channel count is fixed by the first
    call), lengths (S,) device integers or a host sequence, init (S, 4, 4) fp64 or (S, 7) fp32 pose rows -> the refined
    pose (S, 4, 4) fp64, a static buffer that the next call overwrites.  The launch sequence is fixed: the frame's vertex
    map (a memset, 2 launches), its normal map, the model images (a memset, 2 launches), ``iters`` x (``accumulate``,
    ``registration.solve``'s kernel), the push (2 launches); with ``graph=True`` it replays as one graph (DESIGN.md
    section 21.2).  Status words and freezing are ``registration.IcpRefiner``'s: the
    first frame after a reset finds no live slot, freezes in iteration 0 with the few-pairs bit, returns ``init`` bit for
    bit and fills slot 0.  ``register(..., trace=True)`` (``graph=False`` only) also returns the frame's images, the model
    images and, per iteration, clones of the pairs, the summed row, ``delta`` and ``T``.

    Lock step only: per-stream masks, idle streams and restarts inside the graph are out of scope, and ``per_stream=True``
    raises.  ``reset()`` empties every stream's map between calls (two fills, no sync, no new capture)."""

    def __init__(self, streams, capacity, height=64, width=1800, up_fov=3.0, down_fov=-24.8, map_size=4, iters=10, sigma=0.5,
                 max_dist=1.0, kernel_size=5, damping=1e-6, threshold_delta_pose=1e-4, min_pairs=64, graph=True,
                 per_stream=False):
        what = "ProjectiveIcpRefiner"
        if per_stream:
            raise ValueError("%s: lock step only: per-stream masks, idle streams and restarts inside the graph are out of "
                             "scope of the projective refiner (per_stream=True is registration.IcpRefiner's)" % what)
        S, cap, M = stream_count(what, streams, MAX_STREAMS), int(capacity), int(map_size)
        if not 1 <= cap or cap * 4 >= 1 << 31:
            raise ValueError("%s: capacity=%d out of range" % (what, cap))
        H, W, up, down = _image_args(what, height, width, up_fov, down_fov)
        if not 1 <= M <= MAX_SLOTS or S * M > 65535:
            raise ValueError("%s: map_size=%d outside [1, %d] (and streams * map_size <= 65535)" % (what, M, MAX_SLOTS))
        need_iters(what, iters)
        need_sigma(what, sigma)
        need_max_dist(what, max_dist)
        if int(kernel_size) not in KERNEL_SIZES:
            raise ValueError("%s: kernel_size=%r is not instantiated (3 or 5)" % (what, kernel_size))
        need_solver(what, damping, threshold_delta_pose, min_pairs)
        self.streams, self.capacity, self.height, self.width, self.up_fov, self.down_fov = S, cap, H, W, up, down
        self.map_size, self.iters, self.kernel_size = M, int(iters), int(kernel_size)
        self.sigma, self.max_dist, self.damping = float(sigma), float(max_dist), float(damping)
        self.threshold_delta_pose, self.min_pairs, self.graph = float(threshold_delta_pose), int(min_pairs), bool(graph)
        self.per_stream = False
        self.bufs = None
        self.channels = None
        self.replay = Replay(graph)

    # ---- state -------------------------------------------------------------------------------------------------------

    def _alloc(self, device, channels):
        S, M, H, W, cap = self.streams, self.map_size, self.height, self.width, self.capacity
        lib = _lib.load()
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)
        f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=device)
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=device)
        u8 = lambda n: torch.zeros((n,), dtype=torch.uint8, device=device)
        eye = lambda *s: torch.eye(s[-1], dtype=torch.float64, device=device).expand(*s).contiguous()
        G = registration.groups(H * W)
        assert G == lib.icp_accumulate_groups(H * W)
        self.channels = channels
        self.bufs = dict(
            points=f32(S, cap, channels), lengths=i32(S), T=eye(S, 4, 4),
            vertex_ws=u8(lib.proj_vertex_map_workspace_bytes(S, H, W)), vmap=f32(S, H, W, 3), rows=i32(S, H, W),
            nmap=f32(S, H, W, 3), map_v=f32(S, M, H, W, 3), map_n=f32(S, M, H, W, 3),
            model_ws=u8(lib.proj_model_build_workspace_bytes(S, M, H, W)), model_v=f32(S, M, H, W, 3),
            model_n=f32(S, M, H, W, 3), model_src=i32(S, M, H, W), A=eye(S, M, 4, 4), live=i32(S, M), cursor=i32(S),
            partial=f64(S, G, ROW), status=i32(S), iterations=i32(S), pairs=i32(S), cost=f64(S), sum=f64(S, ROW),
            delta=f64(S, 6), slot=i32(S, H, W), pixel=i32(S, H, W))

    status = registration.IcpRefiner.status                 # section 21's words (no stream is ever idle here)
    diagnostics = registration.IcpRefiner.diagnostics

    def map_state(self):
        """Device views of the maps' bookkeeping: A (S, M, 4, 4) the newest frame -> slot, live (S, M), cursor (S,)."""
        if self.bufs is None:
            return None
        return {k: self.bufs[k] for k in ("A", "live", "cursor")}

    def reset(self):
        """Empty every stream's map: the next frame only fills slot 0.  Device fills, no sync, no new capture."""
        if self.bufs is None:
            return
        self.bufs["live"].zero_()
        self.bufs["cursor"].zero_()

    # ---- one registration ----------------------------------------------------------------------------------------------

    def _body(self, trace=None):
        b, S, M, H, W = self.bufs, self.streams, self.map_size, self.height, self.width
        dev, up, down = b["points"].device, self.up_fov, self.down_fov
        _lib.call("proj_vertex_map_kernel_wrapper", dev, S, self.capacity, self.channels, H, W, up, down, _p(b["points"]),
                  _p(b["lengths"]), 0, _p(b["vertex_ws"]), _p(b["vmap"]), _p(b["rows"]))
        _lib.call("proj_normal_map_kernel_wrapper", dev, S, H, W, self.kernel_size, _p(b["vmap"]), _p(b["nmap"]))
        _lib.call("proj_model_build_kernel_wrapper", dev, S, M, H, W, up, down, _p(b["map_v"]), _p(b["map_n"]), _p(b["A"]),
                  _p(b["live"]), _p(b["model_ws"]), _p(b["model_v"]), _p(b["model_n"]), _p(b["model_src"]))
        G = b["partial"].shape[1]
        tracing = trace is not None
        for it in range(self.iters):
            _lib.call("proj_accumulate_kernel_wrapper", dev, S, M, H, W, up, down, _p(b["vmap"]), _p(b["model_v"]),
                      _p(b["model_n"]), _p(b["T"]), self.sigma, self.max_dist, _p(b["partial"]),
                      _p(b["slot"]) if tracing else 0, _p(b["pixel"]) if tracing else 0)
            if tracing:
                before = b["T"].clone()
            _lib.call("icp_solve_kernel_wrapper", dev, S, G, it, _p(b["partial"]), self.damping, self.threshold_delta_pose,
                      self.min_pairs, _p(b["T"]), _p(b["status"]), _p(b["iterations"]), _p(b["pairs"]), _p(b["cost"]),
                      _p(b["sum"]), _p(b["delta"]))
            if tracing:
                trace["steps"].append(dict(slot=b["slot"].clone(), pixel=b["pixel"].clone(), sum=b["sum"].clone(),
                                           delta=b["delta"].clone(), T_before=before, T=b["T"].clone(),
                                           status=b["status"].clone()))
        if tracing:
            trace.update({k: b[k].clone() for k in ("vmap", "rows", "nmap", "model_v", "model_n", "model_src")})
        _lib.call("proj_map_push_kernel_wrapper", dev, S, M, H, W, _p(b["T"]), _p(b["vmap"]), _p(b["nmap"]), _p(b["map_v"]),
                  _p(b["map_n"]), _p(b["A"]), _p(b["live"]), _p(b["cursor"]))

    def _check(self, points, lengths, init):
        what, S = "ProjectiveIcpRefiner", self.streams
        ok = isinstance(points, torch.Tensor) and points.dtype == torch.float32 and points.dim() == 3 and \
            points.shape[0] == S and 1 <= points.shape[1] <= self.capacity and points.shape[2] in (3, 4)
        if not ok:
            raise ValueError("%s: points must be float32 (%d, R <= %d, 3|4), got %s %s"
                             % (what, S, self.capacity, getattr(points, "dtype", type(points)),
                                tuple(getattr(points, "shape", ()))))
        if self.channels is not None and points.shape[2] != self.channels:
            raise ValueError("%s: points have %d channels, the first call fixed %d" % (what, points.shape[2], self.channels))
        init_poses(what, init, S)
        need_cuda(points, init)
        R = points.shape[1]
        if isinstance(lengths, torch.Tensor) and lengths.is_cuda:
            if tuple(lengths.shape) != (S,) or lengths.dtype.is_floating_point or lengths.dtype == torch.bool:
                raise ValueError("%s: lengths must be (%d,) integers, got %s %s" % (what, S, lengths.dtype,
                                                                                  tuple(lengths.shape)))
            return lengths                                  # clamped to [0, R] on the device
        arr = np.asarray(lengths.numpy() if isinstance(lengths, torch.Tensor) else lengths)
        if arr.shape != (S,) or arr.dtype.kind not in "iu":
            raise ValueError("%s: lengths must be (%d,) integers, got %s %s" % (what, S, arr.dtype, arr.shape))
        bad = [int(v) for v in arr if not 0 <= int(v) <= R]
        if bad:
            raise ValueError("%s: lengths %s outside [0, %d] (the rows given)" % (what, bad, R))
        return torch.tensor([int(v) for v in arr], dtype=torch.int32)

    def register(self, points, lengths, init, trace=False):
        if trace and self.graph:
            raise ValueError("ProjectiveIcpRefiner: trace=True needs graph=False (a replayed graph cannot hand out its "
                             "iterations)")
        lengths = self._check(points, lengths, init)
        if init.dim() == 2:
            init = evaluation.rows_to_transforms(init)
        if self.bufs is None:
            self._alloc(points.device, points.shape[2])
        b, R = self.bufs, points.shape[1]
        b["points"][:, :R].copy_(points)
        b["lengths"].copy_(lengths)
        if R < self.capacity:                               # rows past R are never offered
            b["lengths"].clamp_(max=R)
        b["T"].copy_(init)
        out = dict(steps=[]) if trace else None
        self.replay.run(lambda: self._body(out), points.device)
        return (b["T"], out) if trace else b["T"]
