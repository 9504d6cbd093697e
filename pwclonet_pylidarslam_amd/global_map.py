"""The global map on the device: per stream a bank of keyframe clouds and the voxel-hashed map of
their rows at given poses, one point per occupied voxel.

    gm = GlobalMap(streams=S, num_points=8192, voxel_size=0.3)
    gm.advance(cloud, frame_ids, poses)      # banks the frame where frame_id % stride == 0, extends the map
    gm.rebuild(poses)                        # every banked keyframe again, at other poses (after a loop closure)
    xyz = gm.points(0)                       # (min(total, capacity), 3) fp32, the winners in bank order

The rule (``tests/global_map_model.py`` is it in NumPy): row i of keyframe k has the global row id g = k n + i and the world
point ``w = float32(X[bank_frame[k]] p)``; its key is the voxel hash of ``w`` (``preprocess.grid_sample``'s rule); the map
is the ``w`` of the rows with the lowest g of their key, in ascending g.  An older row always beats a newer one, so with
unchanged poses a new keyframe only appends, and extending the map call by call equals rebuilding it, bit for bit.  The
kernels are ``csrc/global_map.hip``; there is no CPU path.
"""
import math

import numpy as np
import torch

from . import _lib, stream_masks
from .stream_engine import need as _need, ptr as _p
from .stream_engine import (Replay, Replayed, frame_ids as _frame_ids, need_cuda, pose_stack, stream_count, stream_index,
                            stream_indices)

MAX_STREAMS = 1024                               # csrc/global_map.hpp: GM_MAX_STREAMS, GM_MAX_KEYFRAMES, GM_MAX_ROWS
MAX_KEYFRAMES = 65535
MAX_ROWS = 1 << 29
BLOCK = 256
WORDS = 8
DEFAULT_CAPACITY = 1 << 22                       # capacity=None of the class: min(MK n, 2^22) rows per stream


def table_slots(max_keyframes, num_points):
    """T: the smallest power of two >= 2 MK n, at least 64."""
    L = 6
    while (1 << L) < 2 * int(max_keyframes) * int(num_points):
        L += 1
    return 1 << L


def map_bytes(S, max_keyframes, num_points, capacity):
    """Bytes of the device buffers of S streams: ``12 T + 8`` of table, ``16 MK n`` of bank and slot words, the bank's
    words, the block counts, the state and ``20 capacity`` of outputs per stream."""
    MK, n = int(max_keyframes), int(num_points)
    T = table_slots(MK, n)
    return int(S) * (8 * T + 4 * (T + 2) + 16 * MK * n + 8 * MK + 4 * MK * ((n + BLOCK - 1) // BLOCK) + 4 * WORDS
                     + 20 * int(capacity))


def _sizes(what, S, MK, n, voxel_size, capacity, stride=1, max_new=1):
    """-> (S, MK, n, voxel_size, capacity); ValueError naming the argument otherwise."""
    S, MK, n = stream_count(what, S, MAX_STREAMS), int(MK), int(n)
    if n < 1:
        raise ValueError("%s: num_points=%d must be >= 1" % (what, n))
    if not 1 <= MK <= MAX_KEYFRAMES:
        raise ValueError("%s: max_keyframes=%d outside [1, %d]" % (what, MK, MAX_KEYFRAMES))
    if MK * n > MAX_ROWS:
        raise ValueError("%s: max_keyframes * num_points = %d above 2^29 (a map that outgrows one table)" % (what, MK * n))
    ok = isinstance(voxel_size, (int, float, np.integer, np.floating)) and not isinstance(voxel_size, bool)
    if not ok or not math.isfinite(float(voxel_size)) or not float(voxel_size) > 0.0:
        raise ValueError("%s: voxel_size=%r must be finite and > 0" % (what, voxel_size))
    if capacity is None:
        capacity = min(MK * n, DEFAULT_CAPACITY)
    if not 1 <= int(capacity) <= MK * n:
        raise ValueError("%s: capacity=%d outside [1, max_keyframes * num_points = %d]" % (what, int(capacity), MK * n))
    if int(stride) < 1:
        raise ValueError("%s: stride=%d must be >= 1" % (what, int(stride)))
    if not 1 <= int(max_new) <= MK:
        raise ValueError("%s: max_new=%d outside [1, max_keyframes = %d]" % (what, int(max_new), MK))
    return S, MK, n, float(voxel_size), int(capacity)


def _buffers(S, MK, n, capacity, device, bank_cloud=None):
    """The device buffers of S streams, empty; ``bank_cloud``: the caller's (S, MK, n, 3) clouds as the bank."""
    T = table_slots(MK, n)
    assert _lib.load().global_map_bytes(S, MK, n, capacity) == map_bytes(S, MK, n, capacity)
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=device)
    state = i32(S, WORDS)
    state[:, 3] = 1                                # dirty: the first insert clears the table
    return dict(keys=torch.zeros((S, T), dtype=torch.int64, device=device), rows=i32(S, T + 2), slots=i32(S, MK, n),
                bank_cloud=torch.zeros((S, MK, n, 3), dtype=torch.float32, device=device) if bank_cloud is None
                else bank_cloud, bank_frame=i32(S, MK),
                bank_len=i32(S, MK), blocks=i32(S, MK, (n + BLOCK - 1) // BLOCK), state=state, overflow=i32(1),
                points=torch.zeros((S, capacity, 3), dtype=torch.float32, device=device), source=i32(S, capacity, 2))


def _map_launches(b, S, MK, n, E, capacity, voxel_size, poses):
    """clear, insert, count, scan, write, end: what follows begin (and push) in every call."""
    dev, frames = poses.device, int(poses.shape[0])
    bank = (_p(b["bank_cloud"]), _p(b["bank_frame"]), _p(b["bank_len"]))
    table = (_p(b["keys"]), _p(b["rows"]))
    _lib.call("global_map_clear_kernel_wrapper", dev, S, MK, n, _p(b["state"]), *table)
    _lib.call("global_map_insert_kernel_wrapper", dev, S, MK, n, E, voxel_size, _p(poses), frames, *bank, _p(b["state"]),
              *table, _p(b["slots"]))
    _lib.call("global_map_count_kernel_wrapper", dev, S, MK, n, E, bank[2], _p(b["state"]), *table, _p(b["slots"]),
              _p(b["blocks"]))
    _lib.call("global_map_scan_kernel_wrapper", dev, S, MK, n, _p(b["state"]), _p(b["blocks"]))
    _lib.call("global_map_write_kernel_wrapper", dev, S, MK, n, E, capacity, _p(poses), frames, *bank, _p(b["state"]), *table,
              _p(b["slots"]), _p(b["blocks"]), _p(b["points"]), _p(b["source"]))
    _lib.call("global_map_end_kernel_wrapper", dev, S, _p(b["state"]))


def _begin(b, S, MK, n, stride, E, mode, dev, active=None, restart=None, frame_id=None, lengths=None):
    _lib.call("global_map_begin_kernel_wrapper", dev, S, MK, n, stride, E, mode, _p(active), _p(restart), _p(frame_id),
              _p(lengths), _p(b["state"]), _p(b["bank_frame"]), _p(b["bank_len"]), _p(b["overflow"]))


# ---- the op alone ------------------------------------------------------------------------------------------------------

def build(clouds, poses, voxel_size, lengths=None, capacity=None):
    """clouds (K, n, 3) fp32, poses (K, 4, 4) fp64 (keyframe k at poses[k]), ``lengths`` (K,) int32 or None (all n rows) ->
    (points (m, 3) fp32, source (m, 2) int32 = (keyframe, row), total): the map of one stream, m = min(total, capacity);
    ``capacity=None``: K n.  Reads ``total`` (a sync)."""
    what = "global_map.build"
    if not isinstance(clouds, torch.Tensor) or clouds.dim() != 3 or clouds.shape[2] != 3 or clouds.shape[0] < 1:
        raise ValueError("%s: clouds must be float32 (K >= 1, n, 3), got %s" % (what, tuple(getattr(clouds, "shape", ()))))
    K, n = int(clouds.shape[0]), int(clouds.shape[1])
    _need(clouds, "%s: clouds" % what, torch.float32, (K, n, 3), cuda=False)
    _need(poses, "%s: poses" % what, torch.float64, (K, 4, 4), cuda=False)
    if lengths is not None:
        _need(lengths, "%s: lengths" % what, torch.int32, (K,), cuda=False)
    _, K, n, voxel_size, capacity = _sizes(what, 1, K, n, voxel_size, K * n if capacity is None else capacity)
    need_cuda(clouds, poses, lengths)
    dev = clouds.device
    b = _buffers(1, K, n, capacity, dev, bank_cloud=clouds.view(1, K, n, 3))
    b["bank_frame"].copy_(torch.arange(K, dtype=torch.int32, device=dev).view(1, K))
    if lengths is None:
        b["bank_len"].fill_(n)
    else:
        b["bank_len"].copy_(lengths.clamp(0, n).view(1, K))
    b["state"][:, 0] = K
    X = poses.view(K, 1, 4, 4)
    _begin(b, 1, K, n, 1, K, 1, dev)
    _map_launches(b, 1, K, n, K, capacity, voxel_size, X)
    total = int(b["state"][0, 2].item())
    m = min(total, capacity)
    return b["points"][0, :m], b["source"][0, :m], total


# ---- the map of S streams ----------------------------------------------------------------------------------------------

class GlobalMap(Replayed):
    """S global maps on the device, one per stream, each over a bank of at most ``max_keyframes`` clouds of ``num_points``
    rows.

    ``advance(cloud, frame_ids, poses, active=None, restart=None, lengths=None)``: cloud (S, n, 3) fp32; frame_ids (S,) int32
    device tensor or host integers; poses (frames, S, 4, 4) fp64, read by frame id inside the launches (a trajectory buffer
    that later calls extend in place; a keyframe whose frame id lies outside it contributes nothing).  Per active stream: a
    ``restart`` empties bank and map first; the frame is banked where ``frame_id % stride == 0`` (a full bank sets the
    overflow word and stores nothing); then at most ``max_new`` of the banked keyframes that are not yet in the map enter
    it, the others wait for the next call.  ``active`` / ``restart``: masks as ``registration.IcpRefiner`` takes them; an
    idle stream keeps every word.  ``lengths`` (S,) int32: only rows [0, lengths[s]) are candidates.  No sync;
    replayed as one graph per poses buffer.

    ``rebuild(poses)``: the map of every banked keyframe at these poses (same launches with ``max_new = max_keyframes``, a
    graph of its own).  ``points(stream)`` / ``sources(stream)``: the first ``min(total, capacity)`` rows, (m, 3) fp32 and
    (m, 2) int32 = (frame id, row) (they read the total: a sync).  ``totals()`` / ``counts()``: (S,) int32 device views of
    the winners (not clamped) and of the banked keyframes; ``built()``: of the keyframes already in the map.
    ``capacity=None``: ``min(max_keyframes * num_points, 2^22)`` rows per stream; winners past it are dropped in order."""

    def __init__(self, streams, num_points, voxel_size=0.3, max_keyframes=1024, capacity=None, stride=1, max_new=1,
                 graph=True, device="cuda"):
        what = "GlobalMap"
        self.streams, self.max_keyframes, self.num_points, self.voxel_size, self.capacity = _sizes(
            what, streams, max_keyframes, num_points, voxel_size, capacity, stride, max_new)
        self.stride, self.max_new, self.graph = int(stride), int(max_new), bool(graph)
        self.device = torch.device(device)
        self.replay = Replay(graph)
        self.bufs = None

    # ---- state -------------------------------------------------------------------------------------------------------

    def _alloc(self):
        S, n, dev = self.streams, self.num_points, self.device
        self.bufs = _buffers(S, self.max_keyframes, n, self.capacity, dev)
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
        self.bufs.update(cloud=torch.zeros((S, n, 3), dtype=torch.float32, device=dev), frame_id=i32(S), lengths=i32(S),
                         active=torch.ones(S, dtype=torch.int32, device=dev), restart=i32(S))

    def map_bytes(self):
        """Bytes of the tables, banks and outputs of all streams (``global_map_bytes`` of the library)."""
        return map_bytes(self.streams, self.max_keyframes, self.num_points, self.capacity)

    def _word(self, k):
        return None if self.bufs is None else self.bufs["state"][:, k]

    def counts(self):
        """(S,) int32 device view: the keyframes banked per stream.  None before the first call."""
        return self._word(0)

    def built(self):
        """(S,) int32 device view: the keyframes already in the map (``counts() - built()`` wait for later calls)."""
        return self._word(1)

    def totals(self):
        """(S,) int32 device view: the winners per stream, not clamped to ``capacity``."""
        return self._word(2)

    def overflowed(self):
        """Whether a full bank ever refused a keyframe (a host read)."""
        return self.bufs is not None and bool(self.bufs["overflow"].item())

    def reset(self, streams=None):
        """Empties the banks and maps of ``streams`` (host indices; None: all, and the overflow word) on the device,
        without a sync."""
        which = stream_indices("GlobalMap", "reset", streams, self.streams)
        if self.bufs is None:
            return
        st = self.bufs["state"]
        for s in which:
            st[s, :3].zero_()
            st[s, 3:4].fill_(1)
        if streams is None:
            self.bufs["overflow"].zero_()

    def invalidate(self, streams=None):
        """Marks the maps of ``streams`` (host indices; None: all) for re-entry and keeps their banks: the table is cleared
        in the next call, and the banked keyframes enter the map again, ``max_new`` per ``advance``, at the poses those
        calls are given: a rebuild spread over the calls that follow.  On the device, without a sync."""
        which = stream_indices("GlobalMap", "invalidate", streams, self.streams)
        if self.bufs is None:
            return
        st = self.bufs["state"]
        for s in which:
            st[s, 1:3].zero_()
            st[s, 3:4].fill_(1)

    def _rows(self, what, stream, name):
        s = stream_index("GlobalMap", what, stream, self.streams)
        if self.bufs is None:
            return None
        m = min(int(self.bufs["state"][s, 2].item()), self.capacity)
        return self.bufs[name][s, :m]

    def points(self, stream):
        """(m, 3) fp32 device view: the map of one stream, m = min(total, capacity).  None before the first call."""
        return self._rows("points", stream, "points")

    def sources(self, stream):
        """(m, 2) int32 device view: (frame id, row) of every map point."""
        return self._rows("sources", stream, "source")

    def bank(self, stream):
        """Device views of one stream's bank: cloud (count, n, 3), frame_id (count,), length (count,) (reads the count)."""
        s = stream_index("GlobalMap", "bank", stream, self.streams)
        b = self.bufs
        c = int(b["state"][s, 0].item())
        return dict(cloud=b["bank_cloud"][s, :c], frame_id=b["bank_frame"][s, :c], length=b["bank_len"][s, :c])

    # ---- launches ----------------------------------------------------------------------------------------------------

    def _body(self, mode, poses):
        b, S, MK, n = self.bufs, self.streams, self.max_keyframes, self.num_points
        E = MK if mode == 1 else self.max_new
        if mode == 0:
            _begin(b, S, MK, n, self.stride, E, 0, self.device, b["active"], b["restart"], b["frame_id"], b["lengths"])
            _lib.call("global_map_push_kernel_wrapper", self.device, S, MK, n, _p(b["cloud"]), _p(b["state"]),
                      _p(b["bank_cloud"]))
        else:
            _begin(b, S, MK, n, self.stride, E, 1, self.device)
        _map_launches(b, S, MK, n, E, self.capacity, self.voxel_size, poses)

    def _run(self, mode, poses):
        self.replay.run(lambda: self._body(mode, poses), self.device, (mode, poses.data_ptr(), int(poses.shape[0])))

    def advance(self, cloud, frame_ids, poses, active=None, restart=None, lengths=None):
        what = "GlobalMap"
        S, n = self.streams, self.num_points
        _need(cloud, "%s: cloud" % what, torch.float32, (S, n, 3), cuda=False)      # every argument's kind and shape first
        given, frame_ids = _frame_ids(what, frame_ids, S)
        pose_stack(what, "poses", poses, S)
        if lengths is not None:
            _need(lengths, "%s: lengths" % what, torch.int32, (S,), cuda=False)
        act = None if active is None else stream_masks.stream_mask(active, S, "active", what)
        rst = None if restart is None else stream_masks.stream_mask(restart, S, "restart", what)
        need_cuda(cloud, given, poses, lengths)
        if self.bufs is None:
            self.device = cloud.device
            self._alloc()
        b = self.bufs
        stream_masks.load_words(b["active"], b["restart"], act, rst)
        b["cloud"].copy_(cloud)
        b["frame_id"].copy_(frame_ids)
        stream_masks.load_lengths(b["lengths"], lengths, n)
        self._run(0, poses)

    def rebuild(self, poses):
        what = "GlobalMap: rebuild"
        pose_stack(what, "poses", poses, self.streams)
        need_cuda(poses)
        if self.bufs is None:
            self.device = poses.device
            self._alloc()
        self._run(1, poses)
