"""Online odometry: one pose per incoming frame, each frame's feature pyramid computed once.

``StreamingOdometry`` runs S independent streams one frame at a time.  Frame k's pyramid (ingest, sampling chain,
set abstractions, kept neighbour-search structures, the early cost-volume products) is computed when frame k arrives;
it serves as frame 2 of pair (k-1, k) at once and as frame 1 of pair (k, k+1) on the next call
(``FusedPWCLONet.stream_step``).  Pair mode (``PWCLONet.forward``) computes every frame's pyramid twice; sequence mode
(``forward_sequence``) needs the whole window first.  The rows are bit for bit the fused pair forward's at batch S.

Every step appends its level-1 poses to trajectories kept on the device (``stream_append_masked_kernel``, fp64):
``relative_poses()[k]`` = quat2mat of pair (k-1, k)'s row (``evaluation.rows_to_transforms``, not inverted),
``trajectory()[k]`` = their product (``evaluation.compute_absolute_poses``), row 0 the identity in both.

One engine runs both modes: a state machine on the device keeps one frame counter per stream and
the handover moves only the streams that advanced, all inside one captured graph per input shape.  ``per_stream=True``
lets every call say which streams delivered a frame and which of those start a new sequence; lock step (the default) is
the same machine with every stream active and none restarting, seen through a host-side view.

``PWCLONetOdometry`` mirrors the reference's ``PoseNetOdometry`` / ``OdometryAlgorithm`` interface for one stream
(``init``, ``process_next_frame``, ``get_relative_poses``, ...); Hydra / OmegaConf configs stay out of scope.
"""
import time

import numpy as np
import torch

from . import _lib, preprocess, stream_masks
from .stream_engine import ptr as _p

MAX_STREAMS = 1024          # stream_append_masked_kernel: one workgroup, one thread per stream
RAW_NUM_POINTS = 8192       # raw mode: points sampled from every sweep's survivors (BASELINE configs[4])


class StreamingOdometry:
    """``StreamingOdometry(net, streams=S)``; ``step(frames)`` with frames (S, n_total, c>=3) fp32 point-major on the
    GPU (``[:, :num_points, :3]`` used; ``num_points`` defaults to the first frame's n_total and is fixed from then on)
    -> pose_params (S, 4, 7) of the pair (previous frame, this frame), ``None`` for the first frame after ``reset()``.

    ``net``: a ``PWCLONet`` in eval mode with its fused weights packed (or packable: ``fused="auto"``); call ``step``
    under ``torch.no_grad()``.  ``graph=True`` replays one captured graph per input shape, which serves the frame
    that primes after ``reset()`` as well (its row is computed against the stale previous frame and discarded); the
    returned pose is then a static buffer that the next step overwrites (clone to keep it), as with
    ``graphed.GraphedForward``.  ``max_frames``: capacity of the device trajectories; ``step`` raises once that many
    frames have been recorded since ``reset()``.

    Raw mode (``sweeps=dict(dataset="kitti360" | "kitti", capacity=131072, near_threshold=30.0, tr=...)``):
    ``step_sweeps(sweeps, lengths)`` takes raw LiDAR sweeps (S, R <= capacity, 4) fp32 on the GPU, stream s using rows
    ``[:lengths[s]]``, and runs filter + compaction + exact sampling to ``num_points`` (default 8192) inside the same
    graph: one capture serves every length.  The clouds are bit for bit
    those of ``preprocess.frames_to_clouds(sweep[None, :length], num_points, dataset, cap=capacity)``;
    ``survivor_counts()`` tells a caller which streams kept fewer than ``num_points`` points.  With ``voxel_size=0.3`` (and
    optionally ``voxel_capacity=24576``) in the dict the kept rows are grid-sampled to one per voxel ahead of the sampler
    (``preprocess.grid_sample``); the clouds are then those of ``frames_to_clouds(...,
    voxel_size=, voxel_capacity=)`` and ``voxel_counts()`` gives the winners per stream before the clamp.  With
    ``deskew=True`` in the dict every sweep is motion-compensated on the device (``preprocess.deskew``, DESIGN.md section
    20) before grid, compaction and sampler: ``step_sweeps(sweeps, lengths, times=...)`` then needs the rows' times, (S, R)
    floating on the sweeps' device (and refuses them otherwise), and the motion is the constant-velocity prior, the
    level-1 pose row this stream registered last: the identity for the first two sweeps of a sequence, the row of pair
    (k-2, k-1) for sweep k.  It lives in a device buffer written after the append, inside the graph; ``motion()`` shows it.
    Per-stream mode: a stream that primes (restart, or no previous frame) and its next sweep get the identity, an idle
    stream keeps its motion, ``reset()`` / ``reset(streams=...)`` return the streams to the identity.

    Refinement (``refine=dict(map_size=4, iters=10, ...)``, ``registration.IcpRefiner``'s keywords; DESIGN.md section 21;
    ``refine=dict(kind="projective", height=64, width=1800, up_fov=3.0, down_fov=-24.8, ...)``: raw mode and lock step only,
    ``projective.ProjectiveIcpRefiner``'s keywords, the dense search-free registration of section 22 on the rows the front
    end keeps; ``kind`` defaults to ``"knn"``):
    after each step's own graph, which is unchanged, the cloud the step sampled from is registered by point-to-plane ICP
    against a local map of the stream's last frames, with the level-1 row's transform as the initial guess (one more
    captured graph).  ``refined_relative_poses()`` / ``refined_trajectory()`` sit beside ``relative_poses()`` /
    ``trajectory()``, which stay the network's, as does the de-skew prior (unless ``feedback=True``, below);
    ``refiner().status()`` tells why a stream's registration stopped.  One path serves both modes: after the step's graph
    the refiner's graph reads the call's ``active`` word and ``restart = active * (1 - valid)`` (a stream that primed in
    this call: a first frame, a ``restart`` mask, ``reset()`` or ``reset(streams=...)``) in place, and one launch records
    the refined pose at the stream's own frame counter, row 0 the identity again after a restart.  No sync, no new
    capture; pose rows, ``relative_poses``, ``trajectory``, ``valid``, ``frame_counts`` and the de-skew prior stay the
    network's.  Per-stream mode opts into the per-stream view inside the dict: ``per_stream=True`` needs
    ``refine=dict(..., per_stream=True)`` (status bit 8 for idle streams) and raises without the key; lock step raises
    with it.  ``refined_relative_poses(stream=i)`` / ``refined_trajectory(stream=i)`` then give (count_i, 4, 4).
    Keyframes: ``refine=dict(..., keyframe=dict(trans=0.1, rot=0.3))`` (metres, degrees) reaches the
    ``"knn"`` refiner in both modes: a frame goes into the local map only when the motion since the stream's last inserted
    frame exceeds a threshold, decided on the device inside the refiner's graph (``refiner().keyframe_state()``).  The
    projective refiner has no keyframe gate yet.
    ``refine=dict(kind="voxel_map", voxel_size=1.0, extent=(128, 128, 32), ...)`` (``voxel_map.VoxelMapRefiner``'s keywords;
    DESIGN.md section 24) registers the same cloud against a persistent voxel map per stream instead of the ring of frames,
    in both modes, with ``keyframe=`` and ``feedback=``.
    ``refine=dict(..., feedback=True)`` (raw mode with ``deskew=True`` only, ``ValueError`` otherwise): after the
    registration one launch writes the refined pose's row into ``motion()`` for the streams that registered a pair in this
    call, so the next sweep is de-skewed with the refined motion instead of the network's; primed and idle streams keep
    their rows.  Pose rows, ``relative_poses()`` and ``trajectory()`` stay the network's in both settings, and without the
    key ``motion()`` holds the bits it always held.

    Global map (``map=dict(voxel_size=0.3, max_keyframes=1024, capacity=None, stride=1, max_new=1, source=...,
    rebuild_on_optimize=True)``, ``global_map.GlobalMap``'s keywords): after the step, the refinement,
    the backend's append and the detector, one more captured graph banks the cloud the step sampled from (every
    ``stride``-th frame of a stream) and extends the stream's map, one point per occupied voxel, at the poses of ``source``:
    ``"optimized"`` (the pose graph's vertices; needs ``backend=``; the default with it), ``"refined"`` (needs ``refine=``)
    or ``"network"``.  It reads the step's words (``active``, ``restart = active * (1 - valid)``, frame ids
    ``frame_counts() - 1``), so dropouts and restarts need no new capture.  ``poll_loops`` rebuilds the map at the corrected
    vertices where the graph was optimised since the map last saw it.  ``global_map()``, ``map_points(stream)``; without
    ``map=`` every path launches what it launched before.

    Localisation in that map (``localize=dict(min_id_distance=200, radius=1, iters=10, sigma=0.5, max_dist=None,
    min_pairs=64, ...)``, ``map_localize.MapLocalizer``'s keywords; needs ``map=``): from the second
    step on, before the map banks the step's frame, an index pass over what the map gained (in full after a rebuild or a
    reset) and one ``localize`` of the step's cloud, the guess the frame's pose in the map's source trajectory and
    ``max_source_frame = frame id - min_id_distance``, so that only old parts of the map attract and a stream that is not
    revisiting freezes with the few-pairs bit.  ``localizer()``, ``localized_pose()``, ``localized_status()``;
    ``poll_localization(optimize=False, information=None)`` (needs ``backend=``) hands the converged fixes to
    ``backend().add_absolute``.  No existing output changes.

    Per-stream mode (``per_stream=True``): ``step(frames, active=None, restart=None)`` and ``step_sweeps(sweeps, lengths,
    active=None, restart=None)`` take two (S,) masks, bool or integer, host sequences or device tensors (device tensors
    are read on the device, without a sync); ``None`` = all active, none restarting.  ``active[s]``: stream s delivered a
    frame in this call (the rows of the other streams are ignored; raw mode: their lengths too, though they must be
    well-formed); ``restart[s]``: that frame starts a new sequence.  Every call returns the static (S, 4, 7) pose, never
    ``None``: a stream's first delivered frame primes that stream alone, and rows that are no real pair (idle or primed
    streams; ``valid()`` tells) hold the identity pose (0,0,0, 1,0,0,0).  A stream that skips calls is paired, when it
    comes back, with the last frame it delivered.  ``frame_counts()``: frames per stream; ``relative_poses(stream=i)`` /
    ``trajectory(stream=i)``: (count_i, 4, 4) of one stream (they read one counter from the device, which may sync);
    without ``stream=`` they raise here, because the streams differ in length.  ``reset(streams=...)`` restarts some
    streams on their next delivered frame.  ``max_frames`` bounds the number of CALLS since the last full ``reset()``:
    the host cannot know the per-stream counts without a sync, and calls >= every count.  One captured graph per input
    shape serves priming, pairs and idling alike: masks, counters and trajectories are device memory that the graph reads.
    Cost: the graph has one shape, so an idle stream costs what an active one does (its row is recomputed from the frame
    it delivered last and discarded); what is gained is correctness under dropouts and restarts with no new capture.  The
    first call (and the first call of every new input shape) needs at least one active stream: idle streams' input rows
    start as copies of the first active stream's, so that no step ever reads an uninitialised buffer."""

    def __init__(self, net, streams=1, num_points=None, max_frames=4096, graph=True, warmup=1, sweeps=None,
                 per_stream=False, refine=None, backend=None, loop=None, map=None, localize=None):
        if not 1 <= int(streams) <= MAX_STREAMS:
            raise ValueError("StreamingOdometry: streams=%d outside [1, %d]" % (int(streams), MAX_STREAMS))
        if int(max_frames) < 1:
            raise ValueError("StreamingOdometry: max_frames=%d must be >= 1" % int(max_frames))
        if num_points is not None and int(num_points) <= 0:
            raise ValueError("StreamingOdometry: num_points=%d must be > 0" % int(num_points))
        self.net, self.streams, self.max_frames = net, int(streams), int(max_frames)
        self.num_points = None if num_points is None else int(num_points)
        self.graph, self.warmup = bool(graph), int(warmup)
        self.frames_seen = 0
        self._slot = None           # persistent buffers of the previous frame (outside every graph pool)
        self._graphs = {}           # input shape (or "sweeps") -> dict(static, step=(graph, pose), cloud)
        self._fused_id = None
        self._rel = self._abs = self._overflow = None
        self.handover_bytes = 0     # bytes the step hands over into the persistent previous frame
        self.per_stream = bool(per_stream)
        self.captures = 0           # graphs captured so far
        self._static = {}           # eager mode: input shape -> static frames (graph mode: in _graphs)
        self._active = self._restart = self._have_prev = self._counts = self._valid = None    # (S,) int32, device
        self._front = None          # raw mode: preprocess.SweepFrontEnd (persistent sweep, lengths, tr, sampler buffers)
        self._refine_cfg = None if refine is None else dict(refine)     # the refiner's keywords
        self._refine_kind = "knn" if refine is None else self._refine_cfg.pop("kind", "knn")
        self._feedback = False if refine is None else self._refine_cfg.pop("feedback", False)
        if not isinstance(self._feedback, (bool, np.bool_)):
            raise ValueError("StreamingOdometry: refine=dict(feedback=%r) must be a bool" % (self._feedback,))
        if self._feedback and not (sweeps is not None and dict(sweeps).get("deskew", False)):
            raise ValueError("StreamingOdometry: refine=dict(feedback=True) hands the refined pose to the de-skew prior and "
                             "needs raw mode with sweeps=dict(..., deskew=True)")
        if self._refine_kind not in ("knn", "projective", "voxel_map"):
            raise ValueError("StreamingOdometry: refine=dict(kind=%r): \"knn\" (registration.IcpRefiner, the default), "
                             "\"projective\" (projective.ProjectiveIcpRefiner) or \"voxel_map\" "
                             "(voxel_map.VoxelMapRefiner)" % (self._refine_kind,))
        if self._refine_kind == "projective":
            if "keyframe" in self._refine_cfg:
                raise ValueError("StreamingOdometry: refine=dict(kind=\"projective\", keyframe=...): the projective refiner "
                                 "has no keyframe gate; keyframe= is registration.IcpRefiner's (kind=\"knn\")")
            if self.per_stream or self._refine_cfg.get("per_stream", False):
                raise ValueError("StreamingOdometry: refine=dict(kind=\"projective\") is lock step only: per-stream masks, "
                                 "idle streams and restarts inside the graph are out of scope (per_stream=True registers "
                                 "with kind=\"knn\")")
            if sweeps is None:
                raise ValueError("StreamingOdometry: refine=dict(kind=\"projective\") registers the rows the sweep front end "
                                 "keeps and needs raw mode: sweeps=dict(...)")
            if dict(sweeps).get("voxel_size") is not None:
                raise ValueError("StreamingOdometry: refine=dict(kind=\"projective\") registers the rows before the grid, "
                                 "which the front end does not keep when voxel_size is set: leave voxel_size out")
        self._refiner = self._ref_rel = self._ref_abs = self._ref_restart = None
        self._backend = None        # backend=: pose_graph.PoseGraph, one vertex per recorded frame
        self._backend_cfg = None if backend is None else dict(backend)
        self._backend_source = None
        if backend is not None:
            self._backend_source = self._backend_cfg.pop("source", "refined" if refine is not None else "network")
            if self._backend_source not in ("refined", "network"):
                raise ValueError("StreamingOdometry: backend=dict(source=%r): \"refined\" or \"network\""
                                 % (self._backend_source,))
            if self._backend_source == "refined" and refine is None:
                raise ValueError("StreamingOdometry: backend=dict(source=\"refined\") takes the refiner's poses and needs "
                                 "refine=dict(...)")
            for key in ("streams", "max_poses", "graph", "device"):
                if key in self._backend_cfg:
                    raise ValueError("StreamingOdometry: backend=dict(%s=...) is the stream's own (streams, max_frames, "
                                     "graph)" % key)
            from .pose_graph import robust_settings             # backend=dict(robust=dict(...)): refused here, not at the first frame
            robust_settings(self._backend_cfg.get("robust"), "StreamingOdometry: backend")
        self._loop = None           # loop=: loop_closure.ScanContextLoopDetector over the step's clouds
        self._loop_cfg = None if loop is None else dict(loop)
        self._loop_restart = self._loop_ids = None
        if loop is not None:
            if backend is None:
                raise ValueError("StreamingOdometry: loop=dict(...) hands its closures to the pose graph and needs "
                                 "backend=dict(...)")
            for key in ("streams", "num_points", "graph", "device"):
                if key in self._loop_cfg:
                    raise ValueError("StreamingOdometry: loop=dict(%s=...) is the stream's own (streams, num_points, graph)"
                                     % key)
        self._map = None            # map=: global_map.GlobalMap over the step's clouds
        self._map_cfg = None if map is None else dict(map)
        self._map_source, self._map_rebuild = None, True
        self._map_restart = self._map_ids = None
        self._map_optimized = 0     # backend().calls when the map was last rebuilt: the optimisations it has seen
        if map is not None:
            default = "optimized" if backend is not None else "refined" if refine is not None else "network"
            self._map_source = self._map_cfg.pop("source", default)
            self._map_rebuild = self._map_cfg.pop("rebuild_on_optimize", True)
            if self._map_source not in ("optimized", "refined", "network"):
                raise ValueError("StreamingOdometry: map=dict(source=%r): \"optimized\", \"refined\" or \"network\""
                                 % (self._map_source,))
            if self._map_source == "optimized" and backend is None:
                raise ValueError("StreamingOdometry: map=dict(source=\"optimized\") places the keyframes at the pose graph's "
                                 "vertices and needs backend=dict(...)")
            if self._map_source == "refined" and refine is None:
                raise ValueError("StreamingOdometry: map=dict(source=\"refined\") places the keyframes at the refiner's "
                                 "poses and needs refine=dict(...)")
            if not isinstance(self._map_rebuild, (bool, np.bool_)):
                raise ValueError("StreamingOdometry: map=dict(rebuild_on_optimize=%r) must be a bool" % (self._map_rebuild,))
            for key in ("streams", "num_points", "graph", "device"):
                if key in self._map_cfg:
                    raise ValueError("StreamingOdometry: map=dict(%s=...) is the stream's own (streams, num_points, graph)"
                                     % key)
            unknown = set(self._map_cfg) - {"voxel_size", "max_keyframes", "capacity", "stride", "max_new"}
            if unknown:
                raise ValueError("StreamingOdometry: map=dict(%s=...): the keys are voxel_size, max_keyframes, capacity, "
                                 "stride, max_new, source, rebuild_on_optimize" % sorted(unknown)[0])
        self._loc = None            # localize=: map_localize.MapLocalizer in the global map
        self._loc_cfg = None if localize is None else dict(localize)
        self._loc_min_id = 200
        self._loc_full = True       # the next step indexes in full (first pass, after a rebuild or a reset)
        self._loc_refill = self._loc_ids = self._loc_newest = None
        self._loc_fresh = False     # a localisation that no poll has looked at yet
        self.localization_dropped = []      # (stream, frame, T, message): fixes the pose graph refused in poll_localization
        if localize is not None:
            if map is None:
                raise ValueError("StreamingOdometry: localize=dict(...) localises in the global map and needs map=dict(...)")
            self._loc_min_id = self._loc_cfg.pop("min_id_distance", 200)
            if isinstance(self._loc_min_id, bool) or not isinstance(self._loc_min_id, (int, np.integer)) \
                    or int(self._loc_min_id) < 1:
                raise ValueError("StreamingOdometry: localize=dict(min_id_distance=%r) must be an integer >= 1"
                                 % (self._loc_min_id,))
            unknown = set(self._loc_cfg) - {"radius", "iters", "sigma", "max_dist", "min_pairs", "min_neighbours", "damping",
                                            "threshold_delta_pose"}
            if unknown:
                raise ValueError("StreamingOdometry: localize=dict(%s=...): the keys are min_id_distance, radius, iters, "
                                 "sigma, max_dist, min_pairs, min_neighbours, damping, threshold_delta_pose"
                                 % sorted(unknown)[0])
        self._tapped = None         # refine / loop / map: the frame batch the last step's graph (or eager step) sampled from
        if refine is not None and self.per_stream != bool(self._refine_cfg.get("per_stream", False)):
            if self.per_stream:
                raise ValueError("StreamingOdometry: per_stream=True registers with the masked refiner, which the refine "
                                 "dict opts into: refine=dict(..., per_stream=True)")
            raise ValueError("StreamingOdometry: refine=dict(per_stream=True) is the masked refiner of per_stream=True; "
                             "lock step registers all streams at once, leave the key out")
        if sweeps is not None:
            if self.num_points is None:
                self.num_points = RAW_NUM_POINTS
            self._front = preprocess.SweepFrontEnd(self.streams, self.num_points, **dict(sweeps))

    # ---- checks --------------------------------------------------------------------------------------------------

    def _check_room(self, what):
        if self.frames_seen >= self.max_frames:           # before any launch: the device trajectories are full
            raise RuntimeError("%s: max_frames=%d frames recorded since reset(); reset() or raise max_frames"
                               % (what, self.max_frames))

    def _check_net(self, x, what):
        net = self.net
        if net.training:
            raise RuntimeError("%s is eval-mode only: call .eval() first" % what)
        if torch.is_grad_enabled():
            raise RuntimeError("%s runs without autograd: call it under torch.no_grad()" % what)
        if net.fuse_mode == "off":
            raise RuntimeError('%s runs on the fused kernels, which config["fused"] = "off" disables' % what)
        if not net._use_fused(x):
            raise RuntimeError("%s: the fused weights are not packed (call prepare_fused() outside capture)" % what)

    def _check(self, frames):
        """The capacity, then forward_sequence's checks and messages, plus the stream's fixed shape.  -> num_points."""
        what = "StreamingOdometry"
        self._check_room(what)
        if not frames.is_cuda:
            raise RuntimeError("CPU not supported")
        if frames.dim() != 3 or frames.dtype != torch.float32:
            raise ValueError("%s: frames must be float32 (S, n_total, c), got %s %s" % (what, frames.dtype,
                                                                                       tuple(frames.shape)))
        S, n_total, c = frames.shape
        if S != self.streams:
            raise ValueError("%s: built for %d streams, got a frame batch of %d" % (what, self.streams, S))
        if c < 3:
            raise ValueError("%s: frames need at least 3 channels (got c=%d)" % (what, c))
        num_points = n_total if self.num_points is None else self.num_points
        if n_total < num_points:
            raise ValueError("%s: frames hold %d points, num_points=%d (fixed when the stream was primed)"
                             % (what, n_total, num_points))
        self._check_net(frames, what)
        return num_points

    # ---- public interface ----------------------------------------------------------------------------------------

    def reset(self, streams=None, tr=None):
        """Start new sequences on all S streams: the next ``step`` primes and returns None.  ``tr``: raw KITTI mode, the
        new sequences' calibration (as ``set_calibration``).  Per-stream mode: ``streams`` restarts those streams alone on
        their next delivered frame, as if that call's ``restart`` named them.  The dtype decides how it is read: integers
        are stream indices (host sequence), booleans an (S,) mask (host sequence or device tensor; a device tensor of
        integers is refused as ambiguous).  Only the streams' ``have_prev`` word is cleared, on the device and without a
        sync, so the mark survives calls in which they idle, and ``frame_counts()``, ``valid()`` and
        ``trajectory(stream=i)`` keep showing the old sequence until that frame arrives.  ``streams=None`` restarts all
        streams at once: counters, ``valid`` and the host call counter that ``max_frames`` bounds are zeroed now."""
        if streams is not None:
            if not self.per_stream:
                raise ValueError("StreamingOdometry: reset(streams=...) needs per_stream=True")
            mask = self._stream_mask(streams)                   # before anything changes
            if tr is not None:
                self.set_calibration(tr)
            if self._have_prev is not None:
                self._have_prev.mul_(1 - mask.to(self._have_prev.device))
            self._reset_motion(mask)
            return
        if tr is not None:
            self.set_calibration(tr)
        if self._have_prev is not None:
            for t in (self._have_prev, self._counts, self._valid):
                t.zero_()
        self.frames_seen = 0
        if self._overflow is not None:
            self._overflow.zero_()
        if self._refiner is not None:
            self._refiner.reset()                           # the maps too
        if self._backend is not None:
            self._backend.reset()                           # the graphs too
        if self._loop is not None:
            self._loop.reset()                              # the places and the closure logs too
        if self._map is not None:
            self._map.reset()                               # the banks and the maps too
            self._loc_full = True
        self._reset_motion(None)

    def _reset_motion(self, mask):
        """The identity motion for the streams of ``mask`` ((S,) int32 0 / 1, anywhere; None: all).  No sync."""
        motion = self.motion()
        if motion is None:
            return
        ident = motion.new_tensor(preprocess.IDENTITY_MOTION).expand_as(motion)
        if mask is None:
            motion.copy_(ident)
        else:
            motion.copy_(torch.where(mask.to(motion.device).ne(0).unsqueeze(1), ident, motion))

    def motion(self):
        """Raw mode with ``deskew=True``: (S, 7) fp32 device view of the pose rows [tx ty tz qw qx qy qz] the streams' next
        sweeps will be de-skewed with (a stream that primes on that sweep gets the identity whatever its row holds).  None
        without ``deskew`` or before the first sweep."""
        if self._front is None or self._front.bufs is None:
            return None
        return self._front.bufs.get("motion")

    @property
    def front(self):
        """Raw mode: the ``preprocess.SweepFrontEnd`` behind ``step_sweeps``; None otherwise."""
        return self._front

    def set_calibration(self, tr):
        """Raw KITTI mode: replace the calibration, (3,4) / (4,4) for all streams or (S,3,4) / (S,4,4) per stream.  It lives
        in a device buffer the captured graphs read, so no new capture follows."""
        if self._front is None:
            raise RuntimeError("StreamingOdometry: set_calibration needs raw mode (sweeps=dict(...))")
        self._front.set_calibration(tr)

    def survivor_counts(self):
        """Raw mode: (S,) int32 device view of the last sweep's survivor counts (min(kept, capacity)); a stream below
        ``num_points`` got index-0 repeats past its count.  None before the first sweep."""
        if self._front is None or self._front.bufs is None:
            return None
        return self._front.bufs["counts"]

    def voxel_counts(self):
        """Raw mode with ``sweeps=dict(..., voxel_size=...)``: (S,) int32 device view of the last sweep's voxel winners per
        stream, not clamped (above ``voxel_capacity`` the later winners were dropped; ``survivor_counts()`` is the clamped
        number).  None without a grid or before the first sweep."""
        return None if self._front is None else self._front.voxel_counts()

    def step(self, frames, active=None, restart=None):
        from . import fused as fused_mod
        self._check_mode(active, restart)
        num_points = self._check(frames)
        act, rst = self._masks(active, restart)
        key = (tuple(frames.shape), frames.device)
        store = self._graphs if self.graph else self._static
        filled = None
        if self._fused_id != id(self.net._fused) or key not in store:
            _, filled = self._seed_idle_rows(act, frames)   # new static rows: idle streams start from an active one
            filled = frames.clone() if filled is frames else filled
        if self.num_points is None:
            self.num_points = num_points       # fixed from the first frame on: the persistent state has its shapes
        fused = self._begin(frames.device)
        stream_masks.load_words(self._active, self._restart, act, rst)
        entry = store.get(key)
        if entry is None:
            entry = store[key] = dict(static=filled, step=None)
        elif act is None:
            entry["static"].copy_(frames)
        else:
            static, src = entry["static"], frames.contiguous()
            per = static[0].numel() * static.element_size()
            fused_mod.masked_copy([(static.data_ptr(), src.data_ptr(), per)], self._active)
        static = entry["static"]
        return self._finish(self._run(fused, entry, self._tap(lambda: static)))

    def step_sweeps(self, sweeps, lengths, times=None, active=None, restart=None):
        """Raw mode: sweeps (S, R <= capacity, 4) fp32 on the GPU, lengths (S,) host integers in [1, R] or a device
        integer tensor (read on the device; clamped to [0, R] there) -> pose as ``step``.  The host copies the rows
        ``[:R]`` and the lengths into static buffers; filter, compaction and sampling run inside the captured graph.
        ``times`` (S, R) floating, on the sweeps' device: the rows' timestamps, required iff the stream was built with
        ``deskew=True`` (ValueError otherwise, before any launch)."""
        what = "StreamingOdometry"
        front = self._front
        if front is None:
            raise RuntimeError("%s: step_sweeps needs raw mode (StreamingOdometry(..., sweeps=dict(dataset=..., "
                               "capacity=...)))" % what)
        front.check_times(times, sweeps, what)
        self._check_mode(active, restart)
        self._check_room(what)
        host_lengths = front.check(sweeps, lengths, what)
        self._check_net(sweeps, what)
        act, rst = self._masks(active, restart)
        if front.bufs is None and act is not None:          # new static rows: idle streams start from an active one
            if host_lengths is None:
                host, sweeps, times, lengths = self._seed_idle_rows(act, sweeps, times, lengths)
            else:
                host, sweeps, times = self._seed_idle_rows(act, sweeps, times)
                first = host_lengths[int(np.flatnonzero(host)[0])]
                host_lengths = [v if a else first for v, a in zip(host_lengths, host)]
        fused = self._begin(sweeps.device)
        stream_masks.load_words(self._active, self._restart, act, rst)
        if front.deskew:
            front.stream_words = (self._restart, self._have_prev)      # read by the front end's launch, on the device
        if front.bufs is None or act is None:
            front.load(sweeps, lengths, host_lengths, times)
        else:
            front.load_masked(sweeps, lengths, host_lengths, self._active, times)
        store = self._graphs if self.graph else self._static
        entry = store.get("sweeps")
        if entry is None:
            entry = store["sweeps"] = dict(static=None, step=None)
        return self._finish(self._run(fused, entry, self._tap(front.run)))

    def relative_poses(self, stream=None):
        """(frames_seen, S, 4, 4) fp64 device view: row 0 the identity, row k the transform of pair (k-1, k).
        Per-stream mode: ``stream=i`` is required and gives that stream's (count_i, 4, 4)."""
        return self._view(self._rel, stream)

    def trajectory(self, stream=None):
        """(frames_seen, S, 4, 4) fp64 device view: the absolute poses, products of ``relative_poses()``; ``stream=i``
        as there."""
        return self._view(self._abs, stream)

    def refined_relative_poses(self, stream=None):
        """With ``refine=``: (frames_seen, S, 4, 4) fp64 device view beside ``relative_poses()``: row k is pair (k-1, k)'s
        transform after point-to-plane registration against the local map, row 0 the identity.
        Per-stream mode: ``stream=i`` is required and gives that stream's (count_i, 4, 4), as ``relative_poses``."""
        return self._view(self._refined(self._ref_rel), stream)

    def refined_trajectory(self, stream=None):
        """With ``refine=``: (frames_seen, S, 4, 4) fp64 device view, the products of ``refined_relative_poses()`` per
        stream, kept on the device as the poses are recorded; ``stream=i`` as there."""
        return self._view(self._refined(self._ref_abs), stream)

    def _refined(self, buf):
        if self._refine_cfg is None:
            raise RuntimeError("StreamingOdometry: refined poses need refine=dict(...)")
        return buf

    def backend(self):
        """With ``backend=``: the ``pose_graph.PoseGraph`` that holds one vertex per recorded frame and stream (``add_loop``,
        ``add_absolute``, ``optimize``); None before the first frame or without ``backend``."""
        return self._backend

    def _need_backend(self):
        if self._backend_cfg is None:
            raise RuntimeError("StreamingOdometry: optimized poses need backend=dict(...)")
        return None if self._backend is None else self._backend.bufs["X"]

    def optimized_trajectory(self, stream=None):
        """With ``backend=``: (frames_seen, S, 4, 4) fp64 device view of the graph's vertices: the source trajectory until
        ``backend().optimize()`` corrects it; ``stream=i`` as ``trajectory``."""
        return self._view(self._need_backend(), stream)

    def optimized_relative_poses(self, stream=None):
        """With ``backend=``: the relative poses of ``optimized_trajectory()``, row 0 the identity, row k = X[k-1]^-1 X[k]
        (device tensor, not a view)."""
        X = self.optimized_trajectory(stream)
        out = torch.eye(4, dtype=torch.float64, device=X.device).expand(X.shape).clone()
        if X.shape[0] > 1:
            Rt = X[:-1, ..., :3, :3].transpose(-1, -2)
            out[1:, ..., :3, :3] = Rt @ X[1:, ..., :3, :3]
            out[1:, ..., :3, 3] = (Rt @ (X[1:, ..., :3, 3] - X[:-1, ..., :3, 3]).unsqueeze(-1)).squeeze(-1)
        return out

    def _backend_append(self, rel):
        """One launch: the graph's vertex of this call's frame, with the step's words (a stream that primed gets an empty
        graph; idle streams keep theirs).  rel: (S, 4, 4) fp64 or (S, 7) fp32 rows."""
        self._backend.append(rel, active=self._active, valid=self._valid, count=self._counts)

    def loop_detector(self):
        """With ``loop=``: the ``loop_closure.ScanContextLoopDetector`` (``match()``, ``loops()``, ``counts()``); None before
        the first frame or without ``loop``."""
        return self._loop

    def _detect(self, pose):
        """After the step, the refinement and the backend's append (outside the step's graph): the detector searches and
        stores the cloud the step sampled from, with the step's own words -- ``active``, ``restart = active * (1 - valid)``
        (a stream that primed starts an empty database, as its graph did), frame ids ``frame_counts() - 1`` -- and the
        backend's vertices as the positions of the distance gate.  No sync."""
        if self._loop_cfg is None:
            return
        if self._loop is None:
            from . import loop_closure
            cfg = dict(self._loop_cfg)
            if "up" not in cfg:     # raw KITTI sweeps come out of the front end in the camera frame
                cfg["up"] = "-y" if self._front is not None and self._front.dataset == "kitti" else "z"
            self._loop = loop_closure.ScanContextLoopDetector(self.streams, self.num_points, graph=self.graph,
                                                              device=pose.device, **cfg)
            self._loop_restart, self._loop_ids = torch.zeros_like(self._active), torch.zeros_like(self._active)
        cloud = self._tapped[:, :self.num_points, :3].contiguous()
        torch.sub(self._active, self._valid, out=self._loop_restart)
        torch.sub(self._counts, 1, out=self._loop_ids)
        self._loop.process(cloud, self._loop_ids, active=self._active, restart=self._loop_restart,
                           trajectory=self._backend.bufs["X"], lengths=self.survivor_counts())      # raw mode: the kept rows

    def poll_loops(self, optimize=False):
        """With ``loop=``: reads the closures the detector accepted since the last poll (a host read) and hands each to
        ``backend().add_loop(stream, i, j, T)``; ``optimize=True`` then runs ``backend().optimize()`` where there was one.
        A stream that primed meanwhile emptied its database and log with its graph, so none of its old records is left;
        a record the graph refuses all the same is kept, with the reason, in ``loop_detector().dropped``.  -> the records
        handed over (``ScanContextLoopDetector.hand_over``)."""
        if self._loop_cfg is None:
            raise RuntimeError("StreamingOdometry: poll_loops needs loop=dict(...)")
        if self._loop is None:
            return []
        added = self._loop.hand_over(self._backend, optimize)
        if self._map is not None and self._map_rebuild and self._map_source == "optimized" \
                and self._backend.calls != self._map_optimized:     # by this poll or by backend().optimize() before it
            self._map.rebuild(self._backend.bufs["X"])      # the keyframes at the corrected vertices
            self._map_optimized = self._backend.calls
            self._loc_full = True                           # the ranks moved: the next step indexes in full
        return added

    def localizer(self):
        """With ``localize=``: the ``map_localize.MapLocalizer`` (``status()``, ``diagnostics()``, ``indexed()``); None until
        the map holds a frame (the second step) or without ``localize``."""
        return self._loc

    def localized_pose(self):
        """With ``localize=``: (S, 4, 4) fp64 device view, the last step's frames localised in the global map; None until
        the map holds a frame."""
        return None if self._loc is None else self._loc.bufs["T"]

    def localized_status(self):
        """With ``localize=``: (S,) int32 device view of the last localisation's status words (``MapLocalizer.status``)."""
        return None if self._loc is None else self._loc.status()

    def _localize(self, pose):
        """After the step, the refinement, the backend's append and the detector, before the map banks the frame: an index
        pass over what the map gained (in full after a rebuild or a reset; from rank 0 for the streams whose map was
        emptied by the last step), then the step's cloud localised in the map with the step's ``active`` word, the frame's
        pose in the map's source trajectory as the guess and ``max_source_frame = frame id - min_id_distance``.  No sync."""
        if self._loc_cfg is None or self._map is None or self._map.bufs is None:
            return                                          # the first step: the map is still empty
        if self._loc is None:
            from . import map_localize
            self._loc = map_localize.MapLocalizer(self._map, graph=self.graph, **self._loc_cfg)
            self._loc_ids, self._loc_newest = torch.zeros_like(self._active), torch.zeros_like(self._active)
        self._loc.index(full=self._loc_full, refill=None if self._loc_full else self._loc_refill)
        self._loc_full = False
        cloud = self._tapped[:, :self.num_points, :3].contiguous()
        torch.sub(self._counts, 1, out=self._loc_ids)
        torch.sub(self._loc_ids, int(self._loc_min_id), out=self._loc_newest)
        X = self._map_poses()
        at = self._loc_ids.clamp(0, X.shape[0] - 1).long()
        init = X[at, torch.arange(self.streams, device=X.device)].contiguous()
        self._loc.localize(cloud, init, active=self._active, max_source_frame=self._loc_newest)
        self._loc_fresh = True

    def poll_localization(self, optimize=False, information=None):
        """With ``localize=`` and ``backend=``: reads the last localisation's words (a host read) and hands the pose of every
        stream whose status is converged with at least ``min_pairs`` pairs to ``backend().add_absolute(stream, frame, T,
        information)``, once per step; ``optimize=True`` then runs ``backend().optimize()`` where an edge was added (and
        the map is rebuilt as ``poll_loops`` rebuilds it).  -> the list of ``(stream, frame, T (4, 4) ndarray)`` handed
        over.  A fix the graph refuses (ValueError: the edge list is full, the pose is not finite) is kept, with the
        reason, in ``localization_dropped`` as ``(stream, frame, T, message)``, as ``loop_detector().dropped`` keeps a
        refused closure."""
        if self._loc_cfg is None:
            raise RuntimeError("StreamingOdometry: poll_localization needs localize=dict(...)")
        if self._backend_cfg is None:
            raise RuntimeError("StreamingOdometry: poll_localization hands absolute edges to the pose graph and needs "
                               "backend=dict(...)")
        if self._loc is None or not self._loc_fresh:
            return []
        self._loc_fresh = False
        status = self._loc.status().cpu().numpy()
        pairs = self._loc.diagnostics()["pairs"].cpu().numpy()
        ids, T = self._loc_ids.cpu().numpy(), self._loc.bufs["T"].cpu().numpy()
        added = []
        for s in range(self.streams):
            if status[s] == 1 and pairs[s] >= self._loc.min_pairs and ids[s] >= 0:
                try:
                    self._backend.add_absolute(s, int(ids[s]), T[s], information)
                except ValueError as e:
                    self.localization_dropped.append((s, int(ids[s]), T[s].copy(), str(e)))
                    continue
                added.append((s, int(ids[s]), T[s].copy()))
        if optimize and added:
            self._backend.optimize()
            if self._map is not None and self._map_rebuild and self._map_source == "optimized":
                self._map.rebuild(self._backend.bufs["X"])
                self._map_optimized = self._backend.calls
                self._loc_full = True
        return added

    def global_map(self):
        """With ``map=``: the ``global_map.GlobalMap`` over the step's clouds (``points``, ``sources``, ``totals``,
        ``rebuild``); None before the first frame or without ``map``."""
        return self._map

    def map_points(self, stream):
        """With ``map=``: (m, 3) fp32 device view of one stream's global map (reads its size: a sync); None before the
        first frame."""
        if self._map_cfg is None:
            raise RuntimeError("StreamingOdometry: map_points needs map=dict(...)")
        return None if self._map is None else self._map.points(stream)

    def _map_poses(self):
        return {"optimized": lambda: self._backend.bufs["X"], "refined": lambda: self._ref_abs,
                "network": lambda: self._abs}[self._map_source]()

    def _extend_map(self, pose):
        """After the step, the refinement, the backend's append and the detector (outside the step's graph): the global map
        banks the cloud the step sampled from and extends itself at the poses of ``map=dict(source=...)``, with the words
        the detector gets: ``active``, ``restart = active - valid``, frame ids ``frame_counts() - 1``, the front end's
        lengths.  No sync."""
        if self._map_cfg is None:
            return
        if self._map is None:
            from . import global_map
            self._map = global_map.GlobalMap(self.streams, self.num_points, graph=self.graph, device=pose.device,
                                             **self._map_cfg)
            self._map_restart, self._map_ids = torch.zeros_like(self._active), torch.zeros_like(self._active)
        cloud = self._tapped[:, :self.num_points, :3].contiguous()
        torch.sub(self._active, self._valid, out=self._map_restart)
        torch.sub(self._counts, 1, out=self._map_ids)
        self._map.advance(cloud, self._map_ids, self._map_poses(), active=self._active, restart=self._map_restart,
                          lengths=self.survivor_counts())
        if self._loc_cfg is not None:                       # the streams whose map this call emptied: indexed from rank 0 next
            if self._loc_refill is None:
                self._loc_refill = torch.zeros_like(self._active)
            self._loc_refill.copy_(self._map_restart)

    def refiner(self):
        """The refiner behind ``refine=``, of the class its ``kind`` names (``status()``, ``diagnostics()``); None before the
        first frame or without ``refine``."""
        return self._refiner

    def valid(self):
        """(S,) int32 device view, 1 where the last call's pose row is a real pair (lock step: all 0 on the call that
        primes, all 1 otherwise).  None before the first call."""
        return self._valid

    def frame_counts(self):
        """(S,) int32 device view of the frames recorded per stream since its last restart (lock step: ``frames_seen``
        for every stream).  None before the first call."""
        return self._counts

    def overflowed(self):
        """Whether the device ever refused an append for lack of capacity (the host check makes this unreachable)."""
        return self._overflow is not None and bool(self._overflow.item())

    # ---- internals ------------------------------------------------------------------------------------------------

    def _begin(self, device):
        """After the checks: the packed weights (a re-pack drops the graphs), the device trajectories."""
        fused = self.net._fused
        if id(fused) != self._fused_id:        # re-packed weights (load_state_dict, prepare_fused): capture again
            self._graphs.clear()
            self._static.clear()
            self._fused_id = id(fused)
        if self._rel is None:
            self._alloc(device)
        if self._backend_cfg is not None and self._backend is None:
            from . import pose_graph
            self._backend = pose_graph.PoseGraph(self.streams, max_poses=self.max_frames, graph=self.graph, device=device,
                                                 **self._backend_cfg)
        return fused

    def _tap(self, source):
        """``source`` itself, or with ``refine=`` a wrapper that remembers the frame batch it returned: the refiner
        registers the cloud the step sampled from.  The step's launches are the same either way."""
        if self._refine_cfg is None and self._loop_cfg is None and self._map_cfg is None:
            return source

        def tapped():
            self._tapped = source()
            return self._tapped
        return tapped

    def _refine(self, pose):
        """After the step (outside its graph): register the step's cloud, initial guess = the level-1 row's transform
        (the identity for a frame that primes), and record the refined relative pose at the stream's own frame counter.
        The refiner reads the step's words: ``active``, and ``restart = active * (1 - valid)`` (a stream that primed in
        this call starts a new map), written as one launch: valid is set for active streams only, so the product is the
        difference.
        ``kind="projective"`` (lock step) registers the rows the front end kept instead -- after the
        filter and the de-skew, packed, before the sampler -- as spherical vertex maps, with the same guess and record."""
        if self._refine_cfg is None:
            return
        if self._refiner is None:
            self._make_refiner(pose.device)
        if self._refine_kind == "projective":
            front = self._front.bufs
            T = self._refiner.register(front["packed"], front["counts"], pose[:, 0, :])
        else:
            cloud = self._tapped[:, :self.num_points, :3].contiguous()
            torch.sub(self._active, self._valid, out=self._ref_restart)
            T = self._refiner.register_adopted(cloud, pose[:, 0, :], all_active=not self.per_stream)
        self._feed_motion(T)
        _lib.call("stream_record_refined_kernel_wrapper", pose.device, self.streams, self.max_frames, _p(self._active),
                  _p(self._valid), _p(self._counts), _p(T), _p(self._ref_rel), _p(self._ref_abs))
        if self._backend_source == "refined":
            self._backend_append(T)

    def _make_refiner(self, device):
        """The refiner of ``refine=dict(kind=...)`` and the refined trajectories.  The two that register the sampled cloud
        read the step's words in place (``adopt_words``)."""
        from . import projective, registration, voxel_map
        if self._refine_kind == "projective":
            self._refiner = projective.ProjectiveIcpRefiner(self.streams, self._front.width, graph=self.graph,
                                                            **self._refine_cfg)
        else:
            make = voxel_map.VoxelMapRefiner if self._refine_kind == "voxel_map" else registration.IcpRefiner
            self._refiner = make(self.streams, self.num_points, graph=self.graph, **self._refine_cfg)
            self._ref_restart = torch.zeros_like(self._active)
            self._refiner.adopt_words(self._active, self._ref_restart)
        self._ref_rel = torch.zeros((self.max_frames, self.streams, 4, 4), dtype=torch.float64, device=device)
        self._ref_abs = torch.zeros_like(self._ref_rel)

    def _feed_motion(self, T):
        """``refine=dict(..., feedback=True)``, one launch after the registration: the streams that registered a pair in
        this call (active and valid) get the pose row of the refined ``T`` as the motion of their next sweep; every other
        row (primed or idle streams) keeps what the step's own handover left."""
        if not self._feedback:
            return
        motion = self.motion()
        _lib.call("stream_motion_from_refined_kernel_wrapper", motion.device, self.streams, _p(self._active),
                  _p(self._valid), _p(T), _p(motion))

    def _view(self, buf, stream=None):
        if stream is None:
            if self.per_stream:
                raise ValueError("StreamingOdometry: per-stream mode keeps trajectories of different lengths; ask for "
                                 "one with stream=i")
            if buf is None:
                return torch.empty((0, self.streams, 4, 4), dtype=torch.float64)
            return buf[:self.frames_seen]
        if not self.per_stream:
            raise ValueError("StreamingOdometry: stream= needs per_stream=True (lock-step trajectories are (frames, S, 4, 4))")
        i = int(stream)
        if not 0 <= i < self.streams:
            raise ValueError("StreamingOdometry: stream=%d outside [0, %d)" % (i, self.streams))
        if buf is None:
            return torch.empty((0, 4, 4), dtype=torch.float64)
        return buf[:int(self._counts[i].item()), i]

    def _alloc(self, device):
        shape = (self.max_frames, self.streams, 4, 4)
        self._rel = torch.zeros(shape, dtype=torch.float64, device=device)
        self._abs = torch.zeros(shape, dtype=torch.float64, device=device)
        self._overflow = torch.zeros((1,), dtype=torch.int32, device=device)
        z = lambda: torch.zeros((self.streams,), dtype=torch.int32, device=device)
        self._active, self._restart, self._have_prev, self._counts, self._valid = z(), z(), z(), z(), z()

    def _hand_motion(self, pose):
        """Raw mode with ``deskew``, after the append, one launch: the motion of the streams' next sweeps = the level-1
        rows of ``pose`` (S, 4, 7), the identity for a stream that primed; streams with ``active[s] == 0`` keep theirs."""
        motion = self.motion()
        if motion is None:
            return
        _lib.call("stream_motion_handover_kernel_wrapper", motion.device, self.streams, _p(self._active), _p(pose),
                  int(pose.stride(0)), _p(motion))

    def _warm(self, fn):
        """Allocator warm-up and one-time kernel attributes on a side stream, as ``GraphedForward`` does."""
        dev = self._rel.device
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), torch.no_grad():
            out = None
            for _ in range(max(1, self.warmup)):
                out = fn()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        return out

    def _capture(self, fn):
        graph = torch.cuda.CUDAGraph()
        with _lib.capture(graph), torch.no_grad():
            out = fn()
        return graph, out

    def _stream_mask(self, mask, what="streams"):
        """``stream_masks.stream_mask`` for this object; ``what == "streams"`` (``reset``): integers are stream indices."""
        return stream_masks.stream_mask(mask, self.streams, what, "StreamingOdometry", indices=what == "streams")

    def _check_mode(self, active, restart):
        if not self.per_stream and (active is not None or restart is not None):
            raise ValueError("StreamingOdometry: active / restart masks need per_stream=True")

    def _masks(self, active, restart):
        """The call's masks, checked (ValueError before any launch) -> ((S,) int32 tensors or None, None)."""
        act = None if active is None else self._stream_mask(active, "active")
        rst = None if restart is None else self._stream_mask(restart, "restart")
        return act, rst

    def _seed_idle_rows(self, act, *tensors):
        return stream_masks.seed_idle_rows(act, self.streams, "StreamingOdometry", *tensors)

    def _append(self, pose):
        """One launch: the per-stream state machine over this call's masks; non-pair rows of ``pose`` become identity."""
        assert pose.is_contiguous() and pose.shape == (self.streams, 4, 7)
        _lib.call("stream_append_masked_kernel_wrapper", pose.device, self.streams, self.max_frames, _p(self._active),
                  _p(self._restart), _p(pose), _p(self._rel), _p(self._abs), _p(self._have_prev), _p(self._counts),
                  _p(self._valid), _p(self._overflow))

    def _body(self, fused, source):
        """The launches of one call, captured or eager: source, the step against the persistent previous frame, the
        masked append, the motion handover, the masked frame-1 handover (ordered after every reader of the previous
        frame: the pair stage has joined its side streams by the time it returns)."""
        pose, new = fused.stream_step(self._slot, source(), self.num_points)
        self._append(pose)
        if self._backend_source == "network":          # the level-1 rows: identity for a stream that is no pair
            self._backend_append(pose[:, 0, :].contiguous())
        self._hand_motion(pose)                        # primed streams' rows are the identity by now
        self._slot.copy_frame1_masked_(new, self._active)
        return pose

    def _run(self, fused, entry, source):
        """``entry``: dict(step=(graph, pose) | None) of this input shape.  Creates the persistent previous frame from a
        real state on the very first call (a step must never read uninitialised search structures), captures once per
        entry, replays (or runs the same launches eagerly)."""
        n = self.num_points
        if self._slot is None:
            prime = lambda: fused.stream_prime(source(), n)
            first = self._warm(prime) if self.graph else prime()
            self._slot = first.frame1_buffers().copy_frame1_(first)
            self.handover_bytes = self._slot.frame1_bytes()
        if not self.graph:
            return self._body(fused, source)
        if entry["step"] is None:
            self._warm(lambda: fused.stream_step(self._slot, source(), n))
            entry["step"] = self._capture(lambda: self._body(fused, source))
            entry["cloud"] = self._tapped              # refine: the batch this graph samples from
            self.captures += 1
        self._tapped = entry["cloud"]
        graph, pose = entry["step"]
        graph.replay()
        return pose

    def _finish(self, pose):
        """After the step: the refinement (a primed stream's rows of ``pose`` are the identity by now); the call
        counter; lock step knows on the host that this call primed every stream (the first since ``reset()``) and
        returns None for it."""
        self._refine(pose)
        self._detect(pose)
        self._localize(pose)
        self._extend_map(pose)
        self.frames_seen += 1
        return None if not self.per_stream and self.frames_seen == 1 else pose


class PWCLONetOdometry:
    """One-stream odometry with the interface of the reference's ``PoseNetOdometry`` (``slam/odometry``):
    ``init()`` loads ``torch.load(checkpoint_path)["prediction_module"]`` and starts a new sequence,
    ``process_next_frame(data_dict)`` reads ``data_dict["numpy_pc"]`` ((n, c) array or tensor) and writes the (4, 4)
    relative pose of (previous frame, this frame) to ``data_dict["odometry_pose"]`` (the identity for the first frame),
    ``get_relative_poses()`` -> (n, 4, 4) float32, first row the identity.  Poses follow ``evaluation``'s convention
    (quat2mat of the level-1 row, not inverted).  Frames need at least ``num_points`` of the prediction config points;
    the first ``num_points`` are used.  With ``sweeps=dict(dataset=..., capacity=..., ...)`` (``StreamingOdometry``'s raw
    mode) ``data_dict["numpy_pc"]`` is instead a raw (n, 4) sweep of any n in [1, capacity], filtered and sampled to
    ``num_points`` on the device.  With ``deskew=True`` in that dict the rows' times come from
    ``data_dict["numpy_pc_timestamps"]`` ((n,) array or tensor; the reference's ``DistortionConfig.timestamps_key``) and
    the sweep is motion-compensated with the last relative pose; a frame without the key passes undistorted, as in the
    reference."""

    def __init__(self, prediction_module_or_config, checkpoint_path=None, device="cuda:0", graph=True,
                 max_frames=4096, sweeps=None, refine=None):
        from .prediction import PWCLONetPredictionModule
        self.device = torch.device(device)
        mod = prediction_module_or_config
        if not isinstance(mod, PWCLONetPredictionModule):
            cfg = dict(mod)
            cfg.setdefault("device", str(self.device))
            mod = PWCLONetPredictionModule(cfg)
        self.prediction_module = mod.to(self.device).eval()
        self.checkpoint_path = checkpoint_path
        self.elapsed = []
        self.stream = StreamingOdometry(mod.pwclonet, streams=1, num_points=mod.num_points, max_frames=max_frames,
                                        graph=graph, sweeps=sweeps, refine=refine)
        self.refine = refine is not None

    def init(self):
        """Start of a sequence: clears the elapsed times and the trajectory, loads the checkpoint if one is given."""
        self.elapsed = []
        if self.checkpoint_path is not None:
            state_dict = torch.load(self.checkpoint_path, map_location=self.device)
            self.prediction_module.load_state_dict(state_dict["prediction_module"])
        self.prediction_module.eval()
        self.stream.reset()

    def process_next_frame(self, data_dict):
        beginning = time.time()
        self.do_process_next_frame(data_dict)
        self.elapsed.append(time.time() - beginning)

    def do_process_next_frame(self, data_dict):
        pc = data_dict[self.input_key()]
        pc = torch.from_numpy(np.ascontiguousarray(pc)) if isinstance(pc, np.ndarray) else pc
        if pc.dim() != 2:
            raise ValueError("PWCLONetOdometry: %s must be one (n, c) frame, got shape %s"
                             % (self.input_key(), tuple(pc.shape)))
        frame = pc.to(self.device, torch.float32)[None]
        with torch.no_grad():
            if self.stream.front is not None:
                self.stream.step_sweeps(frame, [frame.shape[1]], times=self._times(data_dict, frame))
            else:
                self.stream.step(frame)
        poses = self.stream.refined_relative_poses() if self.refine else self.stream.relative_poses()
        data_dict[self.relative_pose_key()] = poses[-1, 0].float().cpu().numpy()

    def _times(self, data_dict, frame):
        """The (1, n) times of a raw frame when the stream de-skews, else None.  A frame without the key gets equal times:
        every alpha is 0 and every row keeps its bits, the identity motion's result (the reference's "no distortion")."""
        if not self.stream.front.deskew:
            return None
        ts = data_dict.get(self.timestamps_key())
        if ts is None:
            return torch.zeros(frame.shape[:2], dtype=torch.float64, device=self.device)
        ts = torch.from_numpy(np.ascontiguousarray(ts)) if isinstance(ts, np.ndarray) else ts
        if ts.numel() != frame.shape[1] or not ts.dtype.is_floating_point:
            raise ValueError("PWCLONetOdometry: %s must hold one floating time per row (%d), got %s %s"
                             % (self.timestamps_key(), frame.shape[1], ts.dtype, tuple(ts.shape)))
        return ts.reshape(1, -1).to(self.device)

    def get_relative_poses(self):
        return self.stream.relative_poses()[:, 0].float().cpu().numpy()

    def get_elapsed(self):
        return sum(self.elapsed)

    @staticmethod
    def input_key():
        return "numpy_pc"

    @staticmethod
    def timestamps_key():
        return "numpy_pc_timestamps"

    @staticmethod
    def pointcloud_key():
        return "odometry_pc"

    @staticmethod
    def relative_pose_key():
        return "odometry_pose"
