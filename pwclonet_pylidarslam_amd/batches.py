"""Training batches from raw LiDAR pairs, built on the device.

The reference makes one training sample in host NumPy inside ``DataLoader`` workers
(``slam/dataset/kitti_odometry_dataset.py:375-463``, ``slam/dataset/kitti_360_dataset_2.py:113-135, 174-272``): both raw
frames cut to the shorter one's row count, calibration transform (KITTI), ground / range filter, a random choice of
``npoints`` survivors (with replacement when there are too few), a random rigid augmentation of frame 2, the dataset's
relative pose composed with that augmentation, and its quaternion.  ``TrainBatchBuilder`` does all of that for a whole batch
in two launches of ``csrc/train_batch.hip`` on persistent buffers and hands over exactly what
``training.PWCLONetWithLoss.forward`` / ``TrainStep`` take.  The random numbers are counter-based (Philox4x32-10 under
``seed``, addressed by row / cloud / step / purpose), so a batch is a function of ``(seed, step, inputs)``: the reference's
NumPy stream is not reproduced, its LAW is, and any step can be replayed.  Lengths, calibration, seed and the step counter
are read from device memory by the launches: one captured graph of ``build`` serves every length and every step.
"""

import numpy as np
import torch

from . import _lib
from .preprocess import KITTI360_GROUND_Z, _calibration

MAX_NPOINTS = 8192             # csrc/train_batch.hip keeps a cloud's selection in LDS: 8192 keys of 8 bytes
MAX_PAIRS = 32767              # one workgroup per cloud, 2 per pair
AUG_SCALE = (0.01, 0.05, 0.01, 0.1, 0.05, 0.5)       # standard deviations of (anglex, angley, anglez, xx, yy, zz) ...
AUG_CLIP = (0.02, 0.1, 0.02, 0.2, 0.15, 1.0)         # ... and their clips; the angles are then multiplied by pi / 4


class TrainBatchBuilder:
    """``build(sweeps (B,2,R,4), lengths (B,2), t_diff (B,4,4) | (B,3,4)) -> (xyz_f1, xyz_f2 (B,3,npoints) f32, gt (B,7) f32)``.

    Pair b = (``sweeps[b, 0]`` = "pc1", ``sweeps[b, 1]`` = "pc2"), rows in scan order; both frames use rows
    ``[:min(lengths[b])]``.  Per cloud: the ``kitti_row`` / ``kitti360_row`` filter of ``preprocess.transform_filter`` /
    ``kitti360_filter`` (same bits), then ``npoints`` survivors: a uniform random subset in random order when there are
    enough, else all survivors in frame order followed by draws with replacement (over all rows when nothing survives).  pc2's
    points are moved by the random rigid ``T_trans`` (fp64, rounded once).  KITTI: ``T_gt = T_diff . inv(T_trans)``, returned
    as ``xyz_f1`` = augmented pc2, ``xyz_f2`` = pc1 (the dataset swaps them); KITTI-360: ``T_gt = T_trans . T_diff``,
    ``xyz_f1`` = pc1, ``xyz_f2`` = augmented pc2.  ``gt = [t_gt, q_gt (w, x, y, z)]``.

    Without ``out=`` the three tensors returned are the builder's own and the next ``build`` overwrites them; with
    ``out=(xyz_f1, xyz_f2, gt)`` the kernels write into the caller's tensors (the static inputs of a graphed ``TrainStep``).
    The kernels read ``sweeps`` where it lies (no copy); ``lengths`` and ``t_diff`` are copied into persistent device buffers
    (under graph capture pass DEVICE tensors for both: a captured copy re-reads them on every replay).  Each ``build`` uses
    the device step counter's current value and leaves it one higher (``step_index`` / ``set_step``; the low 32 bits enter
    the random counter)."""

    def __init__(self, batch, dataset="kitti", npoints=8192, capacity=131072, augment=True, seed=0, near_threshold=30.0,
                 tr=None, ground_z=KITTI360_GROUND_Z):
        if dataset not in ("kitti", "kitti360"):
            raise ValueError("train batch: unknown dataset %r (\"kitti\" or \"kitti360\")" % (dataset,))
        batch, npoints, capacity = int(batch), int(npoints), int(capacity)
        if not 1 <= batch <= MAX_PAIRS:
            raise ValueError("train batch: batch=%d outside [1, %d]" % (batch, MAX_PAIRS))
        if not 1 <= npoints <= MAX_NPOINTS:
            raise ValueError("train batch: npoints=%d outside [1, %d] (a cloud's selection is sorted in LDS)"
                             % (npoints, MAX_NPOINTS))
        if not 1 <= capacity < (1 << 29):
            raise ValueError("train batch: capacity=%d outside [1, 2^29)" % capacity)
        if dataset == "kitti" and tr is None:
            raise ValueError('train batch: dataset="kitti" needs the calibration tr ((3,4) or (B,3,4))')
        seed = int(seed)
        if not -(1 << 63) <= seed < (1 << 64):
            raise ValueError("train batch: seed=%d does not fit 64 bits" % seed)
        self.batch, self.npoints, self.dataset, self.capacity = batch, npoints, dataset, capacity
        self.augment = bool(augment)
        self.seed = seed & ((1 << 64) - 1)
        self.near_threshold, self.ground_z = float(near_threshold), float(ground_z)
        self._tr_host = _calibration(tr, batch) if dataset == "kitti" else None
        self._step_host = 0
        self.bufs = None

    # ---- state -----------------------------------------------------------------------------------------------------------
    def set_calibration(self, tr):
        """Replace the KITTI calibration (per pair or one for all) in place: a captured graph reads the new one."""
        if self.dataset != "kitti":
            raise ValueError("train batch: the KITTI-360 builder takes no calibration")
        self._tr_host = _calibration(tr, self.batch)
        if self.bufs is not None:
            self.bufs["tr"].copy_(self._tr_host)

    def step_index(self):
        """The step the next ``build`` (or replay) will use."""
        return self._step_host if self.bufs is None else int(self.bufs["state"][1].item())

    def set_step(self, k):
        k = int(k)
        if not 0 <= k < (1 << 62):
            raise ValueError("train batch: step=%d outside [0, 2^62)" % k)
        self._step_host = k
        if self.bufs is not None:
            self.bufs["state"][1:2].fill_(k)

    def indices(self):
        """(2B, npoints) int32: the raw row of every output point of cloud 2 * pair + frame (frame 0 = pc1), last build."""
        return self._buf("indices")

    def survivor_counts(self):
        """(2B,) int32: rows of cloud 2 * pair + frame that passed the filter."""
        return self._buf("counts")

    def aug_params(self):
        """(B, 6) fp32: (anglex, angley, anglez, xx, yy, zz) after clipping and the fp32 cast (angles before ``* pi / 4``)."""
        return self._buf("aug")

    def t_gt(self):
        """(B, 4, 4) fp64."""
        return self._buf("t_gt")

    def t_trans(self):
        """(B, 3, 4) fp64: the augmentation applied to pc2 (identity rows when ``augment=False``)."""
        return self._buf("t_trans")

    def _buf(self, name):
        if self.bufs is None:
            raise RuntimeError("train batch: nothing built yet")
        return self.bufs[name]

    # ---- checks (host only) ----------------------------------------------------------------------------------------------
    def check(self, sweeps, lengths, t_diff, out=None, aug=None, what="train batch"):
        """Shape, dtype and value checks of every argument, before any launch.  Returns the host lengths as a (B,2) int32
        tensor, or None for a device tensor (clamped to [0, rows] by the kernel; values are the caller's responsibility)."""
        B, cap, m = self.batch, self.capacity, self.npoints
        if not isinstance(sweeps, torch.Tensor) or sweeps.dim() != 4 or sweeps.dtype != torch.float32:
            raise ValueError("%s: sweeps must be float32 (B, 2, R, 4), got %s %s"
                             % (what, getattr(sweeps, "dtype", type(sweeps)), tuple(getattr(sweeps, "shape", ()))))
        if sweeps.shape[1] != 2 or sweeps.shape[3] != 4:
            raise ValueError("%s: sweeps need 2 frames of 4 channels (x, y, z, intensity) per pair, got %s"
                             % (what, tuple(sweeps.shape)))
        if sweeps.shape[0] != B:
            raise ValueError("%s: built for %d pairs, got a sweep batch of %d" % (what, B, sweeps.shape[0]))
        R = sweeps.shape[2]
        if R > cap:
            raise ValueError("%s: sweeps hold %d rows, capacity=%d" % (what, R, cap))
        if R < 1:
            raise ValueError("%s: sweeps hold no rows" % what)
        host = None
        if isinstance(lengths, torch.Tensor) and lengths.is_cuda:
            if lengths.shape != (B, 2) or lengths.dtype.is_floating_point or lengths.dtype == torch.bool:
                raise ValueError("%s: lengths must be (%d, 2) integers, got %s %s" % (what, B, lengths.dtype,
                                                                                     tuple(lengths.shape)))
        else:
            arr = np.asarray(lengths.numpy() if isinstance(lengths, torch.Tensor) else lengths)
            if arr.shape != (B, 2) or arr.dtype.kind not in "iu":
                raise ValueError("%s: lengths must be (%d, 2) integers, got %s %s" % (what, B, arr.dtype, arr.shape))
            bad = [int(v) for v in arr.reshape(-1) if not 1 <= int(v) <= R]
            if bad:
                raise ValueError("%s: lengths %s outside [1, %d] (the rows given)" % (what, bad, R))
            host = torch.from_numpy(arr.astype(np.int32))
        if not isinstance(t_diff, torch.Tensor):
            t_diff = torch.as_tensor(np.asarray(t_diff))
        if t_diff.dtype != torch.float64 or t_diff.dim() != 3 or t_diff.shape[0] != B or t_diff.shape[1] not in (3, 4) \
                or t_diff.shape[2] != 4:
            raise ValueError("%s: t_diff must be float64 (%d, 4, 4) or (%d, 3, 4), got %s %s"
                             % (what, B, B, t_diff.dtype, tuple(t_diff.shape)))
        if aug is not None:
            if not self.augment:
                raise ValueError("%s: aug= given to a builder made with augment=False" % what)
            if not isinstance(aug, torch.Tensor) or aug.shape != (B, 6) or aug.dtype != torch.float32:
                raise ValueError("%s: aug must be float32 (%d, 6), got %s %s"
                                 % (what, B, getattr(aug, "dtype", type(aug)), tuple(getattr(aug, "shape", ()))))
        if out is not None:
            if len(out) != 3:
                raise ValueError("%s: out must be (xyz_f1, xyz_f2, gt)" % what)
            for name, t, shape in (("xyz_f1", out[0], (B, 3, m)), ("xyz_f2", out[1], (B, 3, m)), ("gt", out[2], (B, 7))):
                if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != shape \
                        or not t.is_contiguous():
                    raise ValueError("%s: out %s must be contiguous float32 %s, got %s %s"
                                     % (what, name, shape, getattr(t, "dtype", type(t)), tuple(getattr(t, "shape", ()))))
                if not t.is_cuda:
                    raise RuntimeError("CPU not supported")
                if t.device != sweeps.device and sweeps.is_cuda:
                    raise ValueError("%s: out %s is on %s, the sweeps on %s" % (what, name, t.device, sweeps.device))
        if not sweeps.is_cuda:
            raise RuntimeError("CPU not supported")
        return host, t_diff

    def _alloc(self, device):
        B, m = self.batch, self.npoints
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)
        seed_signed = self.seed - (1 << 64) if self.seed >= (1 << 63) else self.seed
        b = dict(lengths=e((B, 2), torch.int32), t_diff=e((B, 3, 4), torch.float64),
                 state=torch.tensor([seed_signed, self._step_host, 0], dtype=torch.int64).to(device),
                 aug=torch.zeros((B, 6), dtype=torch.float32, device=device), t_trans=e((B, 3, 4), torch.float64),
                 t_gt=e((B, 4, 4), torch.float64), indices=e((2 * B, m), torch.int32),
                 counts=torch.zeros((2 * B,), dtype=torch.int32, device=device),
                 xyz_f1=e((B, 3, m), torch.float32), xyz_f2=e((B, 3, m), torch.float32), gt=e((B, 7), torch.float32),
                 tr=self._tr_host.to(device) if self.dataset == "kitti" else None)
        self.bufs = b

    # ---- the batch -------------------------------------------------------------------------------------------------------
    def build(self, sweeps, lengths, t_diff, out=None, aug=None):
        host_lengths, t_diff = self.check(sweeps, lengths, t_diff, out, aug)
        _lib.load()                                        # a missing library is an error here, not a fallback
        dev = sweeps.device
        if self.bufs is None:
            self._alloc(dev)
        b = self.bufs
        if b["state"].device != dev:
            raise ValueError("train batch: built on %s, got sweeps on %s" % (b["state"].device, dev))
        sweeps = sweeps.contiguous()
        if sweeps.data_ptr() % 16:
            sweeps = sweeps.clone()
        b["lengths"].copy_(host_lengths if host_lengths is not None else lengths)
        b["t_diff"].copy_(t_diff[:, :3, :])
        mode = 0
        if self.augment:
            mode = 1
            if aug is not None:
                b["aug"].copy_(aug)
                mode = 2
        x1, x2, gt = out if out is not None else (b["xyz_f1"], b["xyz_f2"], b["gt"])
        p = lambda t: t.data_ptr() if t is not None else 0
        ds = 0 if self.dataset == "kitti" else 1
        _lib.call("train_batch_pose_kernel_wrapper", dev, self.batch, ds, mode, p(b["state"]), p(b["t_diff"]), p(b["aug"]),
                  p(b["t_trans"]), p(b["t_gt"]), p(gt))
        _lib.call("train_batch_sample_kernel_wrapper", dev, self.batch, sweeps.shape[2], self.npoints, ds, p(b["lengths"]),
                  p(sweeps), p(b["tr"]), self.ground_z, self.near_threshold, p(b["state"]), p(b["t_trans"]),
                  1 if mode else 0, p(x1), p(x2), p(b["indices"]), p(b["counts"]))
        return x1, x2, gt


def pad_pairs(pairs, capacity=None, device=None):
    """A list of B (pc1 (n1,4), pc2 (n2,4)) float32 array pairs -> (sweeps (B,2,R,4) float32 tensor, zero rows past each
    frame's length; lengths (B,2) int32 tensor), R = capacity or the longest frame.  The host side of feeding ``build``."""
    B = len(pairs)
    R = int(capacity) if capacity is not None else max(max(a.shape[0], c.shape[0]) for a, c in pairs)
    sweeps = torch.zeros((B, 2, R, 4), dtype=torch.float32)
    lengths = torch.zeros((B, 2), dtype=torch.int32)
    for i, pair in enumerate(pairs):
        for f, frame in enumerate(pair):
            n = frame.shape[0]
            if n > R:
                raise ValueError("train batch: a frame of %d rows does not fit capacity=%d" % (n, R))
            sweeps[i, f, :n] = torch.from_numpy(np.ascontiguousarray(frame, dtype=np.float32))
            lengths[i, f] = n
    if device is not None:
        sweeps, lengths = sweeps.to(device), lengths.to(device)
    return sweeps, lengths


def synthetic_raw_pairs(batch, seed=0, capacity=131072, n_azimuth=2048, scenes=8):
    """``batch`` raw-sized synthetic pairs for tools and benchmarks: consecutive sweeps of ``synthetic.raw_sweep_sequence``
    (velodyne frame, scan order, row counts that vary), padded to ``capacity``.  ``scenes`` distinct pairs are ray-cast on
    the host, the rest repeat them (the kernels' work does not depend on which scene a sweep shows).  Returns (sweeps
    (B,2,capacity,4) f32, lengths (B,2) i32, t_diff (B,4,4) f64: the step's motion in the camera frame), host tensors."""
    from . import synthetic
    scenes = min(int(batch), int(scenes))
    frames, q, t = synthetic.raw_sweep_sequence(seed, frames=scenes + 1, n_azimuth=n_azimuth)
    sweeps, lengths = pad_pairs([(frames[i % scenes], frames[i % scenes + 1]) for i in range(batch)], capacity)
    t_diff = torch.eye(4, dtype=torch.float64).repeat(batch, 1, 1)
    for i in range(batch):
        w, x, y, z = (float(v) for v in q[i % scenes])
        t_diff[i, :3, :3] = torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                                          [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                                          [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]],
                                         dtype=torch.float64)
        t_diff[i, :3, 3] = torch.from_numpy(t[i % scenes].astype(np.float64))
    return sweeps, lengths, t_diff


VELO_TO_CAM = ((0.0, -1.0, 0.0, 0.0), (0.0, 0.0, -1.0, 0.0), (1.0, 0.0, 0.0, 0.0))   # the synthetic sweeps' calibration
