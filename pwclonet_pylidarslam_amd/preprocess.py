"""On-device KITTI / KITTI-360 frame preprocessing.

The reference does this in NumPy inside DataLoader workers (``slam/dataset/kitti_odometry_dataset.py``:
``__getitem__`` :375-397 and ``filter_pcd`` :149-172): calibration transform of the raw velodyne
points, ground / range filter, then a random choice of ``npoints`` survivors (with replacement when
there are too few).  Here the transform + filter is one HIP kernel on the raw ``(n, 4)`` frame already
in HBM; compaction and the random choice are torch index ops (the reference's NumPy RNG stream is not
reproducible on the device, so only the deterministic part is bit-comparable), and ``sample="fps"``
replaces the random choice by furthest point sampling (BASELINE.json configs[4]; clouds above
24 576 points use the cooperative multi-workgroup sampler).

KITTI-360 (``slam/dataset/kitti_360_dataset_2.py``: ``filter_pcd`` :113-135) keeps the sensor frame: no
transform, ground = ``z < -(1.73 - 0.3)``, range test on x and y (``kitti360_filter``).  Both filters take
a whole batch of equally long frames ``(b, n, 4)``; ``compact`` packs every frame's survivors to the front
of a zero-padded ``(b, cap, 3)`` batch (zero rows are never selected by the sampler, sampling_gpu.cu:100-101)
and ``frames_to_clouds`` chains filter -> compaction -> one batched furthest-point-sampling call.

``grid_sample`` is the reference's voxel grid filter (``slam/common/pointcloud.py:105-130``): one row per
occupied voxel, the lowest-index one.  It is opt-in (``voxel_size=``) in ``frames_to_clouds`` and the raw-sweep front end.

``deskew`` is the reference's ``distortion`` filter (``slam/preprocessing.py:131-191``): every kept row
moved by its share of a motion prior, the share being its timestamp normalised over the sweep.  Opt-in as well (``times=`` /
``motion=`` in ``frames_to_clouds``, ``deskew=True`` in the raw-sweep front end); it sits between the filter and the grid.
"""
import math
import numbers

import numpy as np
import torch

from . import _lib
from .pointnet2_ops import _ext


KITTI360_GROUND_Z = -(1.73 - 0.3)      # -(VELODYNE_HEIGHT - WHEEL_AXIS_HEIGHT), slam/common/kitti360_utils.py:24-27


def _check_frames(points):
    if not points.is_cuda:
        raise RuntimeError("CPU not supported")
    assert points.dim() in (2, 3) and points.size(-1) == 4 and points.dtype == torch.float32
    return points.contiguous()


def transform_filter(points, tr):
    """points (n,4) or (b,n,4) f32 cuda raw frames sharing one calibration, tr (3,4) or (4,4) array-like
    -> (xyz (...,3) f32, keep (...) i32)."""
    points = _check_frames(points)
    lead = points.shape[:-1]
    n = points.numel() // 4
    tr = torch.as_tensor(tr, dtype=torch.float64).reshape(-1)[:12].contiguous().to(points.device)
    xyz = torch.empty(lead + (3,), dtype=torch.float32, device=points.device)
    keep = torch.empty(lead, dtype=torch.int32, device=points.device)
    _lib.call("kitti_transform_filter_kernel_wrapper", points.device, n, tr.data_ptr(), points.data_ptr(),
              xyz.data_ptr(), keep.data_ptr())
    return xyz, keep


def kitti360_filter(points, near_threshold, ground_z=KITTI360_GROUND_Z):
    """points (n,4) or (b,n,4) f32 cuda raw KITTI-360 frames -> (xyz (...,3) f32, keep (...) i32)."""
    points = _check_frames(points)
    lead = points.shape[:-1]
    xyz = torch.empty(lead + (3,), dtype=torch.float32, device=points.device)
    keep = torch.empty(lead, dtype=torch.int32, device=points.device)
    _lib.call("kitti360_filter_kernel_wrapper", points.device, points.numel() // 4, float(ground_z),
              float(near_threshold), points.data_ptr(), xyz.data_ptr(), keep.data_ptr())
    return xyz, keep


def compact(xyz, keep, cap=None):
    """xyz (b,n,3) f32, keep (b,n) i32 -> (packed (b,cap,3) f32: survivors in frame order, then zero rows;
    counts (b,) i32).  ``cap`` defaults to n (no host sync); survivors beyond cap are dropped."""
    assert xyz.dim() == 3 and keep.shape == xyz.shape[:2] and keep.dtype == torch.int32
    b, n, _ = xyz.shape
    cap = n if cap is None else int(cap)
    xyz = xyz.contiguous()
    keep = keep.contiguous()
    out = torch.zeros((b, cap, 3), dtype=torch.float32, device=xyz.device)
    counts = torch.empty((b,), dtype=torch.int32, device=xyz.device)
    # scan + scatter in one hand-written kernel (csrc/warp.hip: compact_frames_scan_kernel; the scan used to be torch.cumsum)
    _lib.call("compact_frames_scan_kernel_wrapper", xyz.device, b, n, cap, keep.data_ptr(), xyz.data_ptr(),
              out.data_ptr(), counts.data_ptr())
    return out, counts


def _voxel_args(voxel_size, voxel_capacity, capacity, what):
    """Host check of the two grid arguments -> (voxel_size as a float or None, the width of the packed batch)."""
    if voxel_size is None:
        if voxel_capacity is not None:
            raise ValueError("%s: voxel_capacity=%r needs a voxel_size" % (what, voxel_capacity))
        return None, capacity
    if isinstance(voxel_size, bool) or not isinstance(voxel_size, numbers.Real) or not math.isfinite(voxel_size) \
            or not voxel_size > 0:
        raise ValueError("%s: voxel_size=%r must be a finite positive number" % (what, voxel_size))
    if voxel_capacity is None:
        return float(voxel_size), capacity
    if isinstance(voxel_capacity, bool) or not isinstance(voxel_capacity, numbers.Integral) \
            or not 1 <= voxel_capacity <= capacity:
        raise ValueError("%s: voxel_capacity=%r outside [1, capacity=%d]" % (what, voxel_capacity, capacity))
    return float(voxel_size), int(voxel_capacity)


def grid_sample_workspace(b, n, device):
    """The open-addressing table ``grid_sample`` and the raw front end deduplicate through: b clouds of up to n rows."""
    nbytes = _lib.load().grid_sample_workspace_bytes(b, n)
    if nbytes <= 0:
        raise ValueError("grid_sample: no workspace for %d clouds of %d rows (at most 2**20 rows per cloud)" % (b, n))
    return torch.empty((nbytes // 8,), dtype=torch.int64, device=device)


def grid_sample(points, voxel_size, lengths=None, keep=None, workspace=None):
    """Voxel grid sampling (the reference's ``grid_sample`` filter): points (n, 3|4) or (b, n, 3|4)
    f32 cuda -> (keep (b, n) i32: 1 for the lowest-index row of every occupied voxel, counts (b,) i32).  A voxel is the hash
    73856093 qx + 19349669 qy + 83492791 qz (64 bits) of q = rint(double(p) / voxel_size); rows with a non-finite
    coordinate or |p / voxel_size| >= 2^31 are dropped.  ``lengths`` (b,) device integers: only rows [:lengths[c]] of
    cloud c take part; ``keep`` (b, n) i32: only rows with keep != 0 take part (the filters' masks).  The result composes
    with ``compact``.  ``workspace``: a ``grid_sample_workspace(b, n, device)`` to reuse; allocated here otherwise."""
    v, _ = _voxel_args(voxel_size, None, None, "grid_sample")
    if v is None:
        raise ValueError("grid_sample: voxel_size=None must be a finite positive number")
    if not points.is_cuda:
        raise RuntimeError("CPU not supported")
    if points.dim() == 2:
        points = points.unsqueeze(0)
    if points.dim() != 3 or points.size(-1) not in (3, 4) or points.dtype != torch.float32:
        raise ValueError("grid_sample: points must be float32 (n, 3|4) or (b, n, 3|4), got %s %s"
                         % (points.dtype, tuple(points.shape)))
    points = points.contiguous()
    b, n, c = points.shape
    dev = points.device
    keep_out = torch.zeros((b, n), dtype=torch.int32, device=dev)
    counts = torch.zeros((b,), dtype=torch.int32, device=dev)
    if b == 0 or n == 0:
        return keep_out, counts
    if lengths is not None:
        if lengths.shape != (b,) or not lengths.is_cuda or lengths.dtype.is_floating_point or lengths.dtype == torch.bool:
            raise ValueError("grid_sample: lengths must be (%d,) integers on the device" % b)
        lengths = lengths.to(torch.int32).contiguous()
    if keep is not None:
        if keep.dim() == 1:
            keep = keep.unsqueeze(0)
        if keep.shape != (b, n) or keep.dtype != torch.int32 or not keep.is_cuda:
            raise ValueError("grid_sample: keep must be int32 (%d, %d) on the device" % (b, n))
        keep = keep.contiguous()
    if workspace is None:
        workspace = grid_sample_workspace(b, n, dev)
    elif workspace.numel() * workspace.element_size() < _lib.load().grid_sample_workspace_bytes(b, n):
        raise ValueError("grid_sample: the workspace is smaller than grid_sample_workspace(%d, %d)" % (b, n))
    _lib.call("grid_sample_keep_kernel_wrapper", dev, b, n, c, points.data_ptr(),
              lengths.data_ptr() if lengths is not None else 0, keep.data_ptr() if keep is not None else 0, v,
              workspace.data_ptr(), keep_out.data_ptr(), counts.data_ptr())
    return keep_out, counts


IDENTITY_MOTION = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)      # a pose row [tx ty tz qw qx qy qz]


def _times_arg(times, shape, device, what):
    """A (b, n) tensor of row times, floating, where the points are -> fp64 contiguous (fp32 widens exactly)."""
    if not isinstance(times, torch.Tensor) or not times.dtype.is_floating_point:
        raise ValueError("%s: times must be a floating tensor %s, got %s" % (what, tuple(shape), getattr(times, "dtype",
                                                                                                      type(times))))
    if tuple(times.shape) != tuple(shape):
        raise ValueError("%s: times must be %s (one per row), got %s" % (what, tuple(shape), tuple(times.shape)))
    if times.device != device:
        raise ValueError("%s: times live on %s, the rows on %s" % (what, times.device, device))
    return times.to(torch.float64).contiguous()


def deskew(points, times, motion, lengths=None, keep=None):
    """Motion compensation of a sweep (the reference's ``distortion`` filter): points (n, 3|4) or
    (b, n, 3|4) f32 cuda, times (n) or (b, n) fp32 / fp64 (widened exactly), motion (7) or (b, 7) f32 pose rows
    [tx ty tz qw qx qy qz] -> xyz (b, n, 3) f32 with row i moved to R(a_i) p_i + a_i t: a_i = the row's time normalised
    to [0, 1] over the candidates' finite times, R(a) the rotation by a * theta about the motion's axis (slerp from the
    identity).  Candidates are the rows ``[:lengths[c]]`` (``lengths`` (b,) device integers) with ``keep != 0`` (``keep``
    (b, n) i32, the filters' masks); every other row, every row with a_i = 0 and every row under the identity motion keeps
    its bits."""
    if points.dim() == 2:
        points = points.unsqueeze(0)
    if points.dim() != 3 or points.size(-1) not in (3, 4) or points.dtype != torch.float32:
        raise ValueError("deskew: points must be float32 (n, 3|4) or (b, n, 3|4), got %s %s"
                         % (points.dtype, tuple(points.shape)))
    b, n, c = points.shape
    dev = points.device
    if isinstance(times, torch.Tensor) and times.dim() == 1:
        times = times.unsqueeze(0)
    times = _times_arg(times, (b, n), dev, "deskew")
    if not isinstance(motion, torch.Tensor) or motion.dtype != torch.float32 or motion.device != dev:
        raise ValueError("deskew: motion must be a float32 tensor of pose rows on the rows' device")
    if motion.dim() == 1:
        motion = motion.unsqueeze(0)
    if tuple(motion.shape) != (b, 7):
        raise ValueError("deskew: motion must be (%d, 7) pose rows [tx ty tz qw qx qy qz], got %s" % (b, tuple(motion.shape)))
    if not points.is_cuda:
        raise RuntimeError("CPU not supported")
    points, motion = points.contiguous(), motion.contiguous()
    if lengths is not None:
        if lengths.shape != (b,) or not lengths.is_cuda or lengths.dtype.is_floating_point or lengths.dtype == torch.bool:
            raise ValueError("deskew: lengths must be (%d,) integers on the device" % b)
        lengths = lengths.to(torch.int32).contiguous()
    if keep is not None:
        if keep.dim() == 1:
            keep = keep.unsqueeze(0)
        if keep.shape != (b, n) or keep.dtype != torch.int32 or not keep.is_cuda:
            raise ValueError("deskew: keep must be int32 (%d, %d) on the device" % (b, n))
        keep = keep.contiguous()
    xyz = torch.empty((b, n, 3), dtype=torch.float32, device=dev)
    if b == 0 or n == 0:
        return xyz
    _lib.call("deskew_rows_kernel_wrapper", dev, b, n, c, points.data_ptr(), times.data_ptr(), motion.data_ptr(),
              lengths.data_ptr() if lengths is not None else 0, keep.data_ptr() if keep is not None else 0, xyz.data_ptr())
    return xyz


def frames_to_clouds(points, npoints, dataset="kitti", tr=None, near_threshold=30.0, cap=None, voxel_size=None,
                     voxel_capacity=None, times=None, motion=None):
    """A batch of raw frames (b,n,4) -> (clouds (b,npoints,3) f32, counts (b,) i32), deterministic
    (furthest point sampling of each frame's survivors; BASELINE.json configs[4]).  A frame with fewer
    than ``npoints`` survivors gets index-0 repeats past its count exactly as the reference's sampler
    returns them for m > #valid; check ``counts`` when that matters (the dataset's own rule for that case
    is a random draw with replacement, see ``kitti_frame_to_cloud``).  ``voxel_size``: ``grid_sample`` of the filter's
    survivors ahead of the sampler (one point per voxel, frame order); the packed batch is then ``voxel_capacity`` wide
    (default ``cap``) and ``counts`` are the rows that reach the sampler.  ``times`` (b, n) with ``motion`` (b, 7): ``deskew`` of the
    kept rows between the filter and the grid (the keep decision is the filter's, on the coordinates before the step)."""
    assert points.dim() == 3
    width = points.shape[1] if cap is None else int(cap)
    voxel_size, width = _voxel_args(voxel_size, voxel_capacity, width, "frames_to_clouds")
    if (times is None) != (motion is None):
        raise ValueError("frames_to_clouds: times= and motion= come together (de-skewing needs both)")
    if dataset == "kitti":
        xyz, keep = transform_filter(points, tr)
    elif dataset == "kitti360":
        xyz, keep = kitti360_filter(points, near_threshold)
    else:
        raise ValueError(f"unknown dataset {dataset!r}")
    if times is not None:
        xyz = deskew(xyz, times, motion, keep=keep)
    if voxel_size is not None:
        keep, _ = grid_sample(xyz, voxel_size, keep=keep)
        cap = width
    packed, counts = compact(xyz, keep, cap)
    idx = _ext.furthest_point_sampling(packed, npoints)
    clouds = torch.gather(packed, 1, idx.long().unsqueeze(-1).expand(-1, -1, 3))
    return clouds, counts


# ---- raw sweeps of varying length, persistent buffers (StreamingOdometry raw mode) ----------------

_SMALL_CLOUD = 24576            # csrc/sampling.hip: larger clouds go to the cooperative multi-workgroup sampler
_SORTED_CLOUD = 2 * 1024 * 16   # pointnet2_ops/_ext.py: from this size on in the spatial order
_COOP_POINTS = 1024 * 16        # points per workgroup of the cooperative sampler
_COOP_MAX_G = 32                # its workgroups per cloud
_COOP_PLAIN_WGS = 224           # workgroups one plain (graph-capturable) launch of it keeps co-resident
SWEEP_CAPACITY_LIMIT = _COOP_POINTS * _COOP_MAX_G + 1    # capacities below it; the index limit 2^23 is above


def sampler_max_clouds(n):
    """Clouds of ``n`` points one plain launch of the large-cloud sampler takes (csrc/sampling.hip ``coop_launch``: 224
    co-resident workgroups, ceil(n / 16384) per cloud, whole groups of 8 clouds); None: no limit (n <= 24576, the
    register-resident sampler).  More clouds are split over several launches there; the raw stream refuses them."""
    if n <= _SMALL_CLOUD:
        return None
    per = _COOP_PLAIN_WGS // -(-n // _COOP_POINTS)
    return per & ~7 if per >= 8 else per


def _calibration(tr, streams):
    """tr (3,4) / (4,4) for all streams or (S,3,4) / (S,4,4) per stream, array-like -> (S,3,4) fp64 host tensor."""
    t = torch.as_tensor(tr, dtype=torch.float64).cpu()
    if t.dim() == 2:
        t = t.unsqueeze(0).expand(streams, -1, -1)
    if t.dim() != 3 or t.shape[0] != streams or t.shape[1] not in (3, 4) or t.shape[2] != 4:
        raise ValueError("sweeps: tr must be (3,4) / (4,4) or (%d,3,4) / (%d,4,4), got %s"
                         % (streams, streams, tuple(t.shape)))
    return t[:, :3, :].contiguous()


class SweepFrontEnd:
    """Raw sweeps of S streams -> the (S, npoints, 3) clouds ``frames_to_clouds(sweep[None, :length], npoints, dataset,
    cap=capacity)`` gives for each stream, bit for bit, through a fixed set of launches on persistent buffers: one
    ``sweep_filter_compact_kernel`` (filter + compaction of every stream's ``[:length]`` rows, zero rows up to
    ``capacity``, lengths read from the device), then the exact sampler over the (S, capacity, 3) batch writing the
    sampled coordinates itself (no gather).  A captured graph of ``run()`` therefore serves every length up to
    ``capacity``; ``load()`` is the only per-frame host work (two copies).  Host-side checks only until ``load``.

    ``voxel_size``: the first launch becomes ``sweep_filter_grid_compact_kernel`` (filter, then one row per occupied voxel
    of the kept rows as ``grid_sample`` chooses them, then the compaction), and the packed batch is ``voxel_capacity`` wide
    (default ``capacity``; 1 <= voxel_capacity <= capacity): that width, not ``capacity``, decides the sampler kernel, its
    buffers and ``sampler_max_clouds``.  Winners beyond it are dropped in row order; ``voxel_counts()`` is the unclamped
    number per stream.  The clouds are those of ``frames_to_clouds(..., cap=capacity, voxel_size=, voxel_capacity=)``.

    ``deskew=True``: ``load`` / ``load_masked`` also take the rows' times (S, R) into a static
    (S, capacity) fp64 buffer, and the first launch becomes ``sweep_filter_deskew_compact_kernel`` (or its grid form):
    the kept rows are moved by ``deskew``'s rule with the motion in ``bufs["motion"]`` ((S, 7) pose rows on the device,
    the identity to begin with; whoever owns the front end writes it between runs) before grid and compaction.
    ``stream_words = (restart, have_prev)``: (S,) int32 device words of a per-stream state machine; a stream whose
    restart word is set or whose have_prev word is clear gets the identity whatever the buffer holds.  The clouds are
    those of ``frames_to_clouds(..., times=, motion=)``.  With ``deskew=False`` nothing of this exists."""

    def __init__(self, streams, npoints, dataset="kitti360", capacity=131072, tr=None, near_threshold=30.0,
                 ground_z=KITTI360_GROUND_Z, voxel_size=None, voxel_capacity=None, deskew=False):
        if dataset not in ("kitti", "kitti360"):
            raise ValueError("sweeps: unknown dataset %r (\"kitti\" or \"kitti360\")" % (dataset,))
        capacity = int(capacity)
        if not 1 <= capacity < SWEEP_CAPACITY_LIMIT:
            raise ValueError("sweeps: capacity=%d outside [1, %d): at or above the sampler's index limit"
                             % (capacity, SWEEP_CAPACITY_LIMIT))
        voxel_size, width = _voxel_args(voxel_size, voxel_capacity, capacity, "sweeps")
        per = sampler_max_clouds(width)
        if per is not None and streams > per:
            raise ValueError("sweeps: %d streams of capacity %d need %d sampler workgroups each; one plain launch keeps "
                             "only %d such clouds co-resident (fewer streams or a smaller capacity)"
                             % (streams, width, -(-width // _COOP_POINTS), per))
        if dataset == "kitti" and tr is None:
            raise ValueError('sweeps: dataset="kitti" needs the calibration tr ((3,4) or (S,3,4))')
        self.streams, self.npoints, self.dataset, self.capacity = int(streams), int(npoints), dataset, capacity
        self.near_threshold, self.ground_z = float(near_threshold), float(ground_z)
        self.voxel_size, self.width = voxel_size, width        # width of the packed batch: what the sampler sees
        if not isinstance(deskew, (bool, np.bool_)):
            raise ValueError("sweeps: deskew=%r must be True or False" % (deskew,))
        self.deskew = bool(deskew)
        self.stream_words = None                               # per-stream mode: (restart, have_prev) device words
        self._tr_host = _calibration(tr, self.streams) if dataset == "kitti" else None
        self.bufs = None

    def set_calibration(self, tr):
        """Replace the KITTI calibration (per stream or one for all) in place: a captured graph reads the new one."""
        if self.dataset != "kitti":
            raise ValueError("sweeps: the KITTI-360 front end takes no calibration")
        self._tr_host = _calibration(tr, self.streams)
        if self.bufs is not None:
            self.bufs["tr"].copy_(self._tr_host)

    def check(self, sweeps, lengths, what):
        """Shape, dtype and length checks, then the device -> host lengths as a list, or None for a device tensor
        (clamped to [0, rows] by the kernel; values are the caller's responsibility there)."""
        S, cap = self.streams, self.capacity
        if sweeps.dim() != 3 or sweeps.dtype != torch.float32:
            raise ValueError("%s: sweeps must be float32 (S, R, 4), got %s %s" % (what, sweeps.dtype, tuple(sweeps.shape)))
        if sweeps.shape[2] != 4:
            raise ValueError("%s: sweeps need 4 channels (x, y, z, intensity), got c=%d" % (what, sweeps.shape[2]))
        if sweeps.shape[0] != S:
            raise ValueError("%s: built for %d streams, got a sweep batch of %d" % (what, S, sweeps.shape[0]))
        R = sweeps.shape[1]
        if R > cap:
            raise ValueError("%s: sweeps hold %d rows, capacity=%d" % (what, R, cap))
        host = None
        if isinstance(lengths, torch.Tensor) and lengths.is_cuda:
            if lengths.shape != (S,) or lengths.dtype.is_floating_point or lengths.dtype == torch.bool:
                raise ValueError("%s: lengths must be (%d,) integers, got %s %s" % (what, S, lengths.dtype,
                                                                                  tuple(lengths.shape)))
        else:
            arr = np.asarray(lengths.numpy() if isinstance(lengths, torch.Tensor) else lengths)
            if arr.shape != (S,) or arr.dtype.kind not in "iu":
                raise ValueError("%s: lengths must be (%d,) integers, got %s %s" % (what, S, arr.dtype, arr.shape))
            host = [int(v) for v in arr]
            bad = [v for v in host if not 1 <= v <= R]
            if bad:
                raise ValueError("%s: lengths %s outside [1, %d] (the rows given)" % (what, bad, R))
        if not sweeps.is_cuda:
            raise RuntimeError("CPU not supported")
        return host

    def check_times(self, times, sweeps, what):
        """``times`` belongs to ``deskew=True`` and to nothing else: ValueError in both directions, and for a shape other
        than the sweeps' (S, R), a dtype that is not floating or another device.  Before any launch."""
        if not self.deskew:
            if times is not None:
                raise ValueError("%s: times= needs a front end built with deskew=True" % what)
            return
        if times is None:
            raise ValueError("%s: built with deskew=True, so every call needs times= (S, R), one per row" % what)
        if not isinstance(sweeps, torch.Tensor) or sweeps.dim() != 3:
            return                                             # check() refuses the sweeps themselves
        _times_arg(times, sweeps.shape[:2], sweeps.device, what)

    def load(self, sweeps, lengths, host_lengths, times=None):
        """The per-frame host work: rows [:R] into the static sweep buffer, the lengths into the static device lengths
        (and with ``deskew`` the rows' times into the static times)."""
        if self.bufs is None:
            self._alloc(sweeps.device)
        b = self.bufs
        b["sweeps"][:, :sweeps.shape[1]].copy_(sweeps)
        if self.deskew:
            b["times"][:, :sweeps.shape[1]].copy_(times)       # fp32 widens exactly
        if host_lengths is None:
            b["lengths"].copy_(lengths)
        else:
            b["lengths"].copy_(torch.tensor(host_lengths, dtype=torch.int32), non_blocking=False)

    def load_masked(self, sweeps, lengths, host_lengths, active, times=None):
        """``load`` for the streams s with ``active[s] != 0`` only ((S,) int32 on the device, read there; no sync): the
        other streams' static rows and lengths (and times) keep the sweep they delivered last.  One launch."""
        from . import fused
        b, cap = self.bufs, self.capacity
        src = sweeps.contiguous()
        rows = src.shape[1] * 16
        if host_lengths is None:
            new_len = lengths.to(torch.int32).contiguous()
        else:
            new_len = torch.tensor(host_lengths, dtype=torch.int32).to(src.device)
        segments = [(b["sweeps"].data_ptr(), src.data_ptr(), rows), (b["lengths"].data_ptr(), new_len.data_ptr(), 4)]
        dst_strides, src_strides = [cap * 16, 4], [rows, 4]
        if self.deskew:                                        # one more segment of the same copy
            tsrc = times.to(torch.float64).contiguous()
            segments.append((b["times"].data_ptr(), tsrc.data_ptr(), rows // 2))
            dst_strides.append(cap * 8)
            src_strides.append(rows // 2)
        fused.masked_copy(segments, active, dst_strides=dst_strides, src_strides=src_strides)

    def voxel_counts(self):
        """(S,) int32 device view: every stream's voxel winners in the last sweep, not clamped to ``voxel_capacity``
        (``bufs["counts"]`` is the clamped number, the rows that reach the sampler).  None without a grid or before ``load``."""
        return None if self.bufs is None else self.bufs.get("winners")

    def _alloc(self, device):
        S, rows, cap, m = self.streams, self.capacity, self.width, self.npoints
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)
        b = dict(sweeps=torch.zeros((S, rows, 4), dtype=torch.float32, device=device), lengths=e((S,), torch.int32),
                 packed=e((S, cap, 3), torch.float32), counts=torch.zeros((S,), dtype=torch.int32, device=device),
                 idx=e((S, m), torch.int32), tr=None)
        if self.dataset == "kitti":
            b["tr"] = self._tr_host.to(device)
        if self.voxel_size is not None:
            b["grid_ws"] = grid_sample_workspace(S, rows, device)
            b["winners"] = torch.zeros((S,), dtype=torch.int32, device=device)
        if self.deskew:
            b["times"] = torch.zeros((S, rows), dtype=torch.float64, device=device)
            b["motion"] = torch.tensor(IDENTITY_MOTION, dtype=torch.float32).repeat(S, 1).to(device)
        if cap > _SMALL_CLOUD:
            b["tmp"] = e((S, cap), torch.float32)          # the cooperative sampler's exchange workspace
        if cap >= _SORTED_CLOUD:
            lib = _lib.load()
            b["order_ws"] = e((lib.fps_spatial_order_workspace_bytes(S, cap),), torch.uint8)
            b["sorted"] = e((S, cap, 3), torch.float32)
            b["perm"] = e((S, cap), torch.int32)
        self.bufs = b

    def run(self):
        """Filter + compaction + sampling of the loaded sweeps -> a fresh (S, npoints, 3) contiguous fp32 batch."""
        b, S, cap, m = self.bufs, self.streams, self.width, self.npoints
        dev = b["packed"].device
        p = lambda t: t.data_ptr() if t is not None else 0
        if self.deskew:
            restart, have_prev = self.stream_words if self.stream_words is not None else (None, None)
            head = (dev, S, self.capacity, cap, p(b["lengths"]), p(b["sweeps"]), 0 if self.dataset == "kitti" else 1, p(b["tr"]),
                    self.ground_z, self.near_threshold, p(b["times"]), p(b["motion"]), p(restart), p(have_prev))
            if self.voxel_size is None:
                _lib.call("sweep_filter_deskew_compact_kernel_wrapper", *head, p(b["packed"]), p(b["counts"]))
            else:
                _lib.call("sweep_filter_deskew_grid_compact_kernel_wrapper", *head, self.voxel_size, p(b["grid_ws"]),
                          p(b["packed"]), p(b["counts"]), p(b["winners"]))
        elif self.voxel_size is None:
            _lib.call("sweep_filter_compact_kernel_wrapper", dev, S, cap, cap, p(b["lengths"]), p(b["sweeps"]),
                      0 if self.dataset == "kitti" else 1, p(b["tr"]), self.ground_z, self.near_threshold, p(b["packed"]),
                      p(b["counts"]))
        else:
            _lib.call("sweep_filter_grid_compact_kernel_wrapper", dev, S, self.capacity, cap, p(b["lengths"]), p(b["sweeps"]),
                      0 if self.dataset == "kitti" else 1, p(b["tr"]), self.ground_z, self.near_threshold, self.voxel_size,
                      p(b["grid_ws"]), p(b["packed"]), p(b["counts"]), p(b["winners"]))
        clouds = torch.empty((S, m, 3), dtype=torch.float32, device=dev)
        if cap >= _SORTED_CLOUD:
            _lib.call("fps_spatial_order_kernel_wrapper", dev, S, cap, p(b["packed"]), p(b["sorted"]), p(b["perm"]),
                      p(b["order_ws"]))
            _lib.call("furthest_point_sampling_sorted_kernel_wrapper", dev, S, cap, m, p(b["packed"]), p(b["sorted"]),
                      p(b["perm"]), p(b["tmp"]), p(b["idx"]), p(clouds))
        elif cap > _SMALL_CLOUD:
            b["tmp"].fill_(1e10)                           # the single-workgroup fallback's running distances
            _lib.call("furthest_point_sampling_xyz_kernel_wrapper", dev, S, cap, m, p(b["packed"]), p(b["tmp"]),
                      p(b["idx"]), p(clouds))
        else:
            _lib.call("furthest_point_sampling_xyz_kernel_wrapper", dev, S, cap, m, p(b["packed"]), 0, p(b["idx"]),
                      p(clouds))
        return clouds


def kitti_frame_to_cloud(points, tr, npoints, sample="random", generator=None):
    """One raw frame -> (npoints, 3) f32 cloud in the camera frame, as ``KITTIOdometry.filter_pcd`` returns it.
    ``sample``: "random" (the reference's rule, torch RNG) or "fps" (deterministic)."""
    xyz, keep = transform_filter(points, tr)
    indices = keep.nonzero(as_tuple=False).flatten()
    cnt = indices.numel()
    dev = xyz.device
    if sample == "fps":
        cand = xyz[indices] if cnt > 0 else xyz
        if cand.size(0) >= npoints:
            sel = _ext.furthest_point_sampling(cand.unsqueeze(0).contiguous(), npoints)[0].long()
            return cand[sel]
        extra = torch.randint(cand.size(0), (npoints - cand.size(0),), device=dev, generator=generator)
        return torch.cat((cand, cand[extra]))
    if cnt >= npoints:                                   # np.random.choice(indices, npoints, replace=False)
        sel = indices[torch.randperm(cnt, device=dev, generator=generator)[:npoints]]
    elif cnt > 0:                                        # all survivors + a draw with replacement
        sel = torch.cat((indices, indices[torch.randint(cnt, (npoints - cnt,), device=dev, generator=generator)]))
    else:                                                # empty: random over the whole frame (the reference warns)
        sel = torch.randint(xyz.size(0), (npoints,), device=dev, generator=generator)
    return xyz[sel]
