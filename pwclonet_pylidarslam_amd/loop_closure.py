"""Loop detection on the device: Scan Context search that feeds the pose graph.

The reference's detector (``slam/loop_closure.py``, ``ElevationImageLoopClosure``) matches AKAZE features of elevation images
with cv2 and refines with open3d; neither exists here.  This module is the standard LiDAR place recogniser instead (Scan
Context, Kim & Kim, IROS 2018) as HIP kernels: per frame a polar height image, per query an exhaustive circular correlation
against every stored place of the stream (one wave per place, one column shift per lane), the yaw from the best shift, and
``registration.IcpRefiner`` to refine the pose and to decide whether the match is real.

    det = ScanContextLoopDetector(streams=S, num_points=n)
    det.process(cloud, frame_ids, trajectory=pg.bufs["X"])      # once per frame, no sync
    for r in det.loops():                                       # the one host read
        pg.add_loop(r.stream, r.i, r.j, r.T)

The kernels are ``csrc/loop_closure.hip``.  There is no CPU path.
"""
import collections
import math

import numpy as np
import torch

from . import _lib, stream_masks
from .stream_engine import need as _need, ptr as _p
from .stream_engine import (Replay, Replayed, frame_ids as _frame_ids, need_cuda, pose_stack, stream_count, stream_index,
                            stream_indices)

MAX_STREAMS = 1024                                   # csrc/loop_closure.hpp
MAX_RINGS, MIN_SECTORS, MAX_SECTORS = 64, 8, 64
VERIFY_DEFAULTS = dict(iters=20, sigma=0.5, max_dist=2.0, min_fitness=0.3, max_mean_cost=None)
# max_mean_cost=None stands for sigma^2: the refiner's cost is Huber's, r^2 below the knee sigma, so the mean pair of an
# accepted closure lies inside the band the caller declared as inlier noise.  threshold=0.2 is Scan Context's customary one.
# No real LiDAR data was at hand when they were chosen, so neither default is measured.

TRANSLATION_DEFAULTS = dict(cells=128, cell_size=1.0, window=16, yaw_div=2, yaw_half=4, z_step=0.25, tolerance=4,
                            min_agreement=0.5)
EL_RECORD = 8                                        # csrc/elevation.hpp: found, k, a, b, A, occ_Q, occ_E, 0

LoopRecord = collections.namedtuple("LoopRecord", "stream i j T score shift pairs cost")


def _params(what, rings, sectors, max_range, z_offset, up):
    NR, NS = int(rings), int(sectors)
    if not 1 <= NR <= MAX_RINGS:
        raise ValueError("%s: rings=%d outside [1, %d]" % (what, NR, MAX_RINGS))
    if not MIN_SECTORS <= NS <= MAX_SECTORS:
        raise ValueError("%s: sectors=%d outside [%d, %d] (one shift per lane of a wave)" % (what, NS, MIN_SECTORS, MAX_SECTORS))
    if not (float(max_range) > 0.0 and math.isfinite(float(max_range))):
        raise ValueError("%s: max_range=%r must be finite and > 0" % (what, max_range))
    if not math.isfinite(float(z_offset)):
        raise ValueError("%s: z_offset=%r must be finite" % (what, z_offset))
    if up not in ("z", "-y"):
        raise ValueError("%s: up=%r: \"z\" or \"-y\" (KITTI's camera frame)" % (what, up))
    return NR, NS


def tables(rings, sectors, max_range, up="z"):
    """The host tables the kernels read: ring_b (NR,) fp32 = fp32((k max_range / NR)^2) for k = 1..NR, sector_d (NS, 2) fp32
    = fp32(cos, sin)(2 pi s / NS), both computed in fp64, and T0 (NS, 4, 4) fp64: the pose a shift of s sectors starts the
    verification from, Rz(-s 2 pi / NS), for ``up="-y"`` conjugated by the permutation (x, y, z) = (z_cam, -x_cam, -y_cam)."""
    NR, NS = int(rings), int(sectors)
    k = np.arange(1, NR + 1, dtype=np.float64)
    ring_b = ((k * float(max_range) / NR) ** 2).astype(np.float32)
    ang = 2.0 * np.pi * np.arange(NS, dtype=np.float64) / NS
    sector_d = np.stack([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32)
    P = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]]) if up == "-y" else np.eye(3)
    T0 = np.tile(np.eye(4), (NS, 1, 1))
    for s in range(NS):
        c, sn = np.cos(-ang[s]), np.sin(-ang[s])
        T0[s, :3, :3] = P.T @ np.array([[c, -sn, 0.0], [sn, c, 0.0], [0.0, 0.0, 1.0]]) @ P
    return ring_b, sector_d, T0


def _translation(what, translation):
    """The checked ``translation=dict(...)`` with its defaults filled in; ValueError for anything else."""
    unknown = set(translation) - set(TRANSLATION_DEFAULTS)
    if unknown:
        raise ValueError("%s: translation=dict(%s=...): the keys are %s" % (what, sorted(unknown)[0], sorted(TRANSLATION_DEFAULTS)))
    t = dict(TRANSLATION_DEFAULTS, **translation)
    whole = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
    for key, lo, hi in (("cells", 8, 128), ("window", 0, 16), ("yaw_div", 1, 8), ("yaw_half", 0, 8), ("tolerance", 1, 255)):
        if not whole(t[key]) or not lo <= t[key] <= hi:
            raise ValueError("%s: translation=dict(%s=%r): an integer in [%d, %d]" % (what, key, t[key], lo, hi))
        t[key] = int(t[key])
    if t["cells"] % 2:
        raise ValueError("%s: translation=dict(cells=%d) must be even" % (what, t["cells"]))
    for key in ("cell_size", "z_step"):
        v = float(np.float32(t[key]))                   # the kernels' fp32 value must itself be finite and > 0
        if not (v > 0.0 and math.isfinite(v)):
            raise ValueError("%s: translation=dict(%s=%r) must be finite and > 0" % (what, key, t[key]))
        t[key] = float(t[key])
    if not 0.0 <= float(t["min_agreement"]) <= 1.0:
        raise ValueError("%s: translation=dict(min_agreement=%r) outside [0, 1]" % (what, t["min_agreement"]))
    t["min_agreement"] = float(t["min_agreement"])
    return t


def elevation_tables(sectors, yaw_div, yaw_half, up="z"):
    """The host tables of the translation search, computed in fp64, row ``shift * Y + k`` with Y = 2 yaw_half + 1: rot (NS Y, 2)
    fp32 = fp32(cos, sin)(theta) and pose (NS Y, 4, 4) fp64 = [Rz(theta), 0] (for ``up="-y"`` conjugated as ``tables`` does),
    theta = -(shift + (k - yaw_half) / yaw_div) 2 pi / NS: the sign of ``T0``."""
    NS, Y = int(sectors), 2 * int(yaw_half) + 1
    rot = np.zeros((NS * Y, 2), dtype=np.float32)
    pose = np.tile(np.eye(4), (NS * Y, 1, 1))
    P = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]]) if up == "-y" else np.eye(3)
    for s in range(NS):
        for k in range(Y):
            theta = -(float(s) + float(k - int(yaw_half)) / float(yaw_div)) * (2.0 * np.pi) / float(NS)
            c, sn = np.cos(theta), np.sin(theta)
            rot[s * Y + k] = c, sn
            pose[s * Y + k, :3, :3] = P.T @ np.array([[c, -sn, 0.0], [sn, c, 0.0], [0.0, 0.0, 1.0]]) @ P
    return rot, pose


def _check_cloud(what, cloud, S=None, n=None, cuda=True):
    if not isinstance(cloud, torch.Tensor) or cloud.dim() != 3 or cloud.shape[2] != 3 or cloud.dtype != torch.float32 \
            or (S is not None and tuple(cloud.shape) != (S, n, 3)):
        raise ValueError("%s: cloud must be float32 (%s, %s, 3), got %s %s"
                         % (what, "S" if S is None else S, "n" if n is None else n, getattr(cloud, "dtype", type(cloud)),
                            tuple(getattr(cloud, "shape", ()))))
    if cuda:
        need_cuda(cloud)
    if not cloud.is_contiguous():
        raise ValueError("%s: cloud must be contiguous" % what)
    if cloud.shape[0] < 1 or cloud.shape[0] > MAX_STREAMS or cloud.shape[1] < 1:
        raise ValueError("%s: cloud of %d streams and %d points: streams in [1, %d], points >= 1"
                         % (what, cloud.shape[0], cloud.shape[1], MAX_STREAMS))


def scan_context(cloud, rings=20, sectors=60, max_range=80.0, z_offset=2.0, up="z", lengths=None):
    """cloud (S, n, 3) fp32 -> (D, Dn, mask): D (S, NR, NS) fp32 the highest ``z + z_offset`` of every polar cell (0: empty),
    Dn its columns divided by their norms, mask (S,) int64 the non-empty columns.  ``lengths`` (S,) int32 device tensor: only
    the rows [0, lengths[s]) of stream s count."""
    NR, NS = _params("scan_context", rings, sectors, max_range, z_offset, up)
    _check_cloud("scan_context", cloud)
    S, n = cloud.shape[:2]
    if lengths is not None:
        _need(lengths, "scan_context: lengths", torch.int32, (S,))
    dev = cloud.device
    ring_b, sector_d, _ = tables(NR, NS, max_range, up)
    ring_b, sector_d = torch.from_numpy(ring_b).to(dev), torch.from_numpy(sector_d).to(dev)
    D = torch.empty((S, NR, NS), dtype=torch.float32, device=dev)
    Dn = torch.empty_like(D)
    mask = torch.empty((S,), dtype=torch.int64, device=dev)
    _lib.call("scan_context_build_kernel_wrapper", dev, S, n, NR, NS, int(up == "-y"), float(z_offset), _p(cloud),
              _p(lengths), _p(ring_b), _p(sector_d), _p(D), _p(Dn), _p(mask), 0, 0, 0, 0, 0)
    return D, Dn, mask


class ScanContextLoopDetector(Replayed):
    """S loop detectors on the device, one per stream, each with a database of at most ``max_keyframes`` places.

    ``process(cloud, frame_ids, active=None, restart=None, trajectory=None, lengths=None)``: cloud (S, n, 3) fp32, frame_ids
    (S,) int32 device tensor or host integers.  Per active stream: the frame's descriptor; its distance to every stored
    place that is eligible (``frame_id + min_id_distance <= f`` and, where ``trajectory`` (frames, S, 4, 4) fp64 is given and
    ``max_distance`` is not None, the positions read by frame id closer than ``max_distance``); the best place is a match
    where its distance is below ``threshold``; the match is verified (below) and an accepted closure appended to the
    stream's log; then the frame is stored where ``f % stride == 0``.  ``active`` / ``restart``: masks as
    ``registration.IcpRefiner`` takes them; a stream with ``restart`` loses its places and its log before the search, an
    idle one keeps every word of its database and log.  No sync; replayed as one graph per trajectory buffer (DESIGN.md
    section 21.2).

    ``verify=dict(iters=20, sigma=0.5, max_dist=2.0, min_fitness=0.3, max_mean_cost=None)`` (None: ``sigma ** 2``): a private
    ``IcpRefiner(map_size=1, per_stream=True)`` registers the matched place's stored cloud (fetched by the device-side
    index) and then the query from ``T0 = Rz(-shift 2 pi / sectors)``; accepted where the refiner kept moving (status bits 2
    and 4 clear), ``pairs >= min_fitness n`` and ``cost / pairs <= max_mean_cost``.  The logged ``T`` is the pose of the
    query frame j in the stored frame i: ``PoseGraph.add_loop(stream, i, j, T)``.  ``verify=None`` logs ``T0`` for every
    match and keeps no clouds.  Translation is not searched: a revisit outside the refiner's ``max_dist`` basin is rejected.

    ``match()``: device views of the last call's record; ``loops(stream=None)``: the accepted records (the one host read);
    ``counts()``, ``overflowed()``, ``reset(streams=None)``, ``map_bytes()``."""

    def __init__(self, streams, num_points, rings=20, sectors=60, max_range=80.0, z_offset=2.0, up="z", max_keyframes=1024,
                 max_loops=256, stride=1, min_id_distance=200, max_distance=None, threshold=0.2, verify=VERIFY_DEFAULTS,
                 graph=True, device="cuda", translation=None):
        what = "ScanContextLoopDetector"
        S, n, MK, ML = stream_count(what, streams, MAX_STREAMS), int(num_points), int(max_keyframes), int(max_loops)
        if n < 1:
            raise ValueError("%s: num_points=%d must be >= 1" % (what, n))
        NR, NS = _params(what, rings, sectors, max_range, z_offset, up)
        if not 1 <= MK <= 1 << 20 or ML < 1:
            raise ValueError("%s: max_keyframes=%d outside [1, 2^20] or max_loops=%d < 1" % (what, MK, ML))
        if int(stride) < 1 or int(min_id_distance) < 0:
            raise ValueError("%s: stride=%d must be >= 1 and min_id_distance=%d >= 0" % (what, int(stride), int(min_id_distance)))
        if max_distance is not None and not (float(max_distance) > 0.0 and math.isfinite(float(max_distance))):
            raise ValueError("%s: max_distance=%r must be None or finite and > 0" % (what, max_distance))
        if not math.isfinite(float(threshold)):
            raise ValueError("%s: threshold=%r must be finite" % (what, threshold))
        if verify is not None:
            unknown = set(verify) - set(VERIFY_DEFAULTS)
            if unknown:
                raise ValueError("%s: verify=dict(%s=...): the keys are %s" % (what, sorted(unknown)[0], sorted(VERIFY_DEFAULTS)))
            verify = dict(VERIFY_DEFAULTS, **verify)
            if verify["max_mean_cost"] is None and float(verify["sigma"]) > 0.0:
                verify["max_mean_cost"] = float(verify["sigma"]) ** 2
            if not 64 <= n <= 16384:
                raise ValueError("%s: verify registers with IcpRefiner, whose num_points lie in [64, 16384] (got %d); "
                                 "verify=None reports the yaw alone" % (what, n))
            if int(verify["iters"]) < 1 or not float(verify["sigma"]) > 0.0 or not float(verify["max_dist"]) >= 0.0:
                raise ValueError("%s: verify needs iters >= 1, sigma > 0 and max_dist >= 0" % what)
            if not 0.0 <= float(verify["min_fitness"]) <= 1.0 or not float(verify["max_mean_cost"] or 0.0) >= 0.0:
                raise ValueError("%s: verify needs min_fitness in [0, 1] and max_mean_cost >= 0" % what)
        if translation is not None:
            if verify is None:
                raise ValueError("%s: translation= images the stored clouds, which only verify= keeps" % what)
            translation = _translation(what, translation)
        self.translation = translation
        self.streams, self.num_points, self.rings, self.sectors = S, n, NR, NS
        self.max_range, self.z_offset, self.up = float(max_range), float(z_offset), up
        self.max_keyframes, self.max_loops, self.stride, self.min_id_distance = MK, ML, int(stride), int(min_id_distance)
        self.max_distance = None if max_distance is None else float(max_distance)
        self.threshold, self.verify, self.graph = float(threshold), verify, bool(graph)
        self.device = torch.device(device)
        self.replay = Replay(graph)
        self.bufs = None
        self._refiner = None
        self._cursor = [0] * S                      # loops(): nothing; poll(): the records already handed out
        self._epoch = [0] * S
        self.dropped = []                           # hand_over(): (record, why the graph refused it)

    # ---- state -------------------------------------------------------------------------------------------------------

    def _alloc(self):
        S, n, NR, NS, MK, ML, dev = (self.streams, self.num_points, self.rings, self.sectors, self.max_keyframes,
                                     self.max_loops, self.device)
        _lib.load()
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
        f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
        i64 = lambda *s: torch.zeros(s, dtype=torch.int64, device=dev)
        ring_b, sector_d, T0 = tables(NR, NS, self.max_range, self.up)
        self.bufs = dict(
            ring_b=torch.from_numpy(ring_b).to(dev), sector_d=torch.from_numpy(sector_d).to(dev),
            T0_table=torch.from_numpy(T0).to(dev), cloud=f32(S, n, 3), lengths=i32(S), frame_id=i32(S),
            active=torch.ones(S, dtype=torch.int32, device=dev), restart=i32(S), D=f32(S, NR, NS), Dn=f32(S, NR, NS),
            qmask=i64(S), db_desc=f32(S, MK, NS, NR), db_mask=i64(S, MK), db_frame=i32(S, MK), count=i32(S), epoch=i32(S),
            overflow=i32(1), scores=f32(S, MK), shifts=i32(S, MK), match=i32(S, 4), match_score=f32(S), found=i32(S),
            T0=torch.eye(4, dtype=torch.float64, device=dev).expand(S, 4, 4).contiguous(), slot=i32(S),
            log_i=i32(S, ML, 4), log_T=f64(S, ML, 4, 4), log_c=f64(S, ML, 2), nlog=i32(S), log_overflow=i32(1),
            accepted=i32(S), eye=torch.eye(4, dtype=torch.float64, device=dev).expand(S, 4, 4).contiguous())
        if self.verify is not None:
            self.bufs.update(db_cloud=f32(S, MK, n, 3), staging=f32(S, n, 3))
        if self.translation is not None:
            t = self.translation
            G, Y, side = t["cells"], 2 * t["yaw_half"] + 1, 2 * t["window"] + 1
            rot, pose = elevation_tables(NS, t["yaw_div"], t["yaw_half"], self.up)
            self.bufs.update(ei_rot=torch.from_numpy(rot).to(dev), ei_pose=torch.from_numpy(pose).to(dev),
                             ei_img=torch.zeros((S, 1 + Y, G, G), dtype=torch.uint8, device=dev), ei_occ=i32(S, 1 + Y),
                             ei_list=i32(S, Y, G * G), ei_A=i32(S, Y, side, side), ei_record=i32(S, EL_RECORD),
                             T1=torch.eye(4, dtype=torch.float64, device=dev).expand(S, 4, 4).contiguous())

    def map_bytes(self):
        """Bytes of the databases and logs of all streams (96 KiB of cloud per place at n = 8192 with verification) and,
        with ``translation``, of the images, lists and scores of one call (per stream, not per place)."""
        S, n, MK, ML = self.streams, self.num_points, self.max_keyframes, self.max_loops
        per_place = self.rings * self.sectors * 4 + 8 + 4 + (n * 12 if self.verify is not None else 0)
        per_call = 0
        if self.translation is not None:
            t = self.translation
            G, Y, side = t["cells"], 2 * t["yaw_half"] + 1, 2 * t["window"] + 1
            per_call = (1 + Y) * (G * G + 4) + Y * G * G * 4 + Y * side * side * 4 + EL_RECORD * 4 + 128
        return S * (MK * per_place + ML * (16 + 128 + 16) + per_call)

    def counts(self):
        """(S,) int32 device view: the places stored per stream.  None before the first call."""
        return None if self.bufs is None else self.bufs["count"]

    def overflowed(self):
        """Whether a full database or a full log ever refused a write (a host read)."""
        if self.bufs is None:
            return False
        return bool(self.bufs["overflow"].item()) or bool(self.bufs["log_overflow"].item())

    def reset(self, streams=None):
        """Empties the databases and logs of ``streams`` (host indices; None: all) on the device, without a sync."""
        which = stream_indices("ScanContextLoopDetector", "reset", streams, self.streams)
        if self.bufs is None:
            return
        b = self.bufs
        for s in which:
            b["count"][s:s + 1].zero_()
            b["nlog"][s:s + 1].zero_()
            b["epoch"][s:s + 1].add_(1)
        if streams is None:
            b["overflow"].zero_()
            b["log_overflow"].zero_()

    def match(self):
        """Device views of the last call's record per stream: found, entry (-1: no place was eligible), frame_i, shift,
        score, T0 (S, 4, 4) and accepted.  None before the first call."""
        if self.bufs is None:
            return None
        b = self.bufs
        m = b["match"]
        return dict(found=m[:, 0], entry=m[:, 1], frame_i=m[:, 2], shift=m[:, 3], score=b["match_score"], T0=b["T0"],
                    accepted=b["accepted"])

    def seed(self):
        """With ``translation``: device views of the last call's translation search per stream: found, k (the yaw
        candidate), a, b (the offset in cells), A (its agreement), occ_q, occ_e (the non-empty cells of the two images) and T1
        (S, 4, 4), the pose the verification started from (``T0`` where nothing was found).  None before the first call or
        without ``translation``."""
        if self.bufs is None or self.translation is None:
            return None
        r = self.bufs["ei_record"]
        return dict(found=r[:, 0], k=r[:, 1], a=r[:, 2], b=r[:, 3], A=r[:, 4], occ_q=r[:, 5], occ_e=r[:, 6], T1=self.bufs["T1"])

    def database(self, stream):
        """Device tensors of one stream's places: Dn (count, NR, NS), mask (count,), frame_id (count,) and, with
        verification, cloud (count, n, 3) (reads the count: a sync)."""
        s = stream_index("ScanContextLoopDetector", "database", stream, self.streams)
        b = self.bufs
        c = int(b["count"][s])
        out = dict(Dn=b["db_desc"][s, :c].transpose(1, 2), mask=b["db_mask"][s, :c], frame_id=b["db_frame"][s, :c])
        if self.verify is not None:
            out["cloud"] = b["db_cloud"][s, :c]
        return out

    def _records(self, s, start):
        b = self.bufs
        n = int(b["nlog"][s])
        if n <= start:
            return []
        li, lT, lc = b["log_i"][s, start:n].cpu().numpy(), b["log_T"][s, start:n].cpu().numpy(), \
            b["log_c"][s, start:n].cpu().numpy()
        return [LoopRecord(s, int(li[k, 0]), int(li[k, 1]), lT[k].copy(), float(lc[k, 0]), int(li[k, 2]), int(li[k, 3]),
                           float(lc[k, 1])) for k in range(n - start)]

    def loops(self, stream=None):
        """The accepted closures of one stream or of all, as a list of ``LoopRecord(stream, i, j, T, score, shift, pairs,
        cost)``: frame j is frame i again and ``T`` (4, 4) fp64 is the pose of j in i.  The one host read."""
        which = stream_indices("ScanContextLoopDetector", "loops", None if stream is None else [stream], self.streams)
        if self.bufs is None:
            return []
        return [r for s in which for r in self._records(s, 0)]

    def poll(self):
        """The closures accepted since the last ``poll`` (a stream emptied meanwhile starts again at its first record)."""
        if self.bufs is None:
            return []
        epochs = self.bufs["epoch"].cpu().tolist()
        out = []
        for s in range(self.streams):
            if epochs[s] != self._epoch[s]:
                self._epoch[s], self._cursor[s] = epochs[s], 0
            new = self._records(s, self._cursor[s])
            self._cursor[s] += len(new)
            out += new
        return out

    def hand_over(self, pose_graph, optimize=False):
        """``poll()``, then ``pose_graph.add_loop(stream, i, j, T)`` for every new record; ``optimize``: one
        ``pose_graph.optimize()`` afterwards where an edge was added.  A record the graph refuses (ValueError: its stream primed
        meanwhile so the frames are gone, the edge list is full, ``T`` is not finite) is kept in ``self.dropped`` as
        ``(record, message)``, never lost silently.  -> the records added."""
        added = []
        for r in self.poll():
            try:
                pose_graph.add_loop(r.stream, r.i, r.j, r.T)
            except ValueError as e:
                self.dropped.append((r, str(e)))
                continue
            added.append(r)
        if optimize and added:
            pose_graph.optimize()
        return added

    # ---- launches ----------------------------------------------------------------------------------------------------

    def build(self):
        b = self.bufs
        _lib.call("scan_context_build_kernel_wrapper", self.device, self.streams, self.num_points, self.rings, self.sectors,
                  int(self.up == "-y"), self.z_offset, _p(b["cloud"]), _p(b["lengths"]), _p(b["ring_b"]), _p(b["sector_d"]),
                  _p(b["D"]), _p(b["Dn"]), _p(b["qmask"]), _p(b["active"]), _p(b["restart"]), _p(b["count"]), _p(b["nlog"]),
                  _p(b["epoch"]))

    def score(self, trajectory=None):
        b = self.bufs
        gate = trajectory is not None and self.max_distance is not None
        _lib.call("loop_score_kernel_wrapper", self.device, self.streams, self.rings, self.sectors, self.max_keyframes,
                  _p(b["Dn"]), _p(b["qmask"]), _p(b["db_desc"]), _p(b["db_mask"]), _p(b["db_frame"]), _p(b["count"]),
                  _p(b["active"]), _p(b["frame_id"]), self.min_id_distance, _p(trajectory) if gate else 0,
                  int(trajectory.shape[0]) if gate else 0, self.max_distance if gate else 0.0, _p(b["scores"]),
                  _p(b["shifts"]))

    def select(self):
        b = self.bufs
        _lib.call("loop_select_kernel_wrapper", self.device, self.streams, self.sectors, self.max_keyframes, self.stride,
                  self.threshold, _p(b["scores"]), _p(b["shifts"]), _p(b["db_frame"]), _p(b["count"]), _p(b["active"]),
                  _p(b["frame_id"]), _p(b["T0_table"]), _p(b["match"]), _p(b["match_score"]), _p(b["found"]), _p(b["T0"]),
                  _p(b["slot"]), _p(b["overflow"]))

    def fetch(self):
        b = self.bufs
        _lib.call("loop_fetch_kernel_wrapper", self.device, self.streams, self.num_points, self.max_keyframes, _p(b["found"]),
                  _p(b["match"]), _p(b["db_cloud"]), _p(b["staging"]))

    def image(self):
        b, t = self.bufs, self.translation
        _lib.call("elevation_image_kernel_wrapper", self.device, self.streams, self.num_points, self.sectors, t["cells"],
                  2 * t["yaw_half"] + 1, int(self.up == "-y"), self.z_offset, t["cell_size"], t["z_step"], _p(b["cloud"]),
                  _p(b["staging"]), _p(b["lengths"]), _p(b["found"]), _p(b["match"]), _p(b["ei_rot"]), _p(b["ei_img"]),
                  _p(b["ei_occ"]), _p(b["ei_list"]))

    def agreement(self):
        b, t = self.bufs, self.translation
        _lib.call("elevation_score_kernel_wrapper", self.device, self.streams, t["cells"], 2 * t["yaw_half"] + 1, t["window"],
                  t["tolerance"], _p(b["found"]), _p(b["ei_img"]), _p(b["ei_occ"]), _p(b["ei_list"]), _p(b["ei_A"]))

    def choose(self):
        b, t = self.bufs, self.translation
        _lib.call("elevation_choose_kernel_wrapper", self.device, self.streams, self.sectors, 2 * t["yaw_half"] + 1,
                  t["window"], t["tolerance"], int(self.up == "-y"), t["min_agreement"], t["cell_size"], _p(b["found"]),
                  _p(b["match"]), _p(b["ei_A"]), _p(b["ei_occ"]), _p(b["ei_pose"]), _p(b["T0"]), _p(b["ei_record"]),
                  _p(b["T1"]))

    def translate(self):
        """Image, score and choose alone: the three launches of the translation search, after ``fetch``."""
        self.image()
        self.agreement()
        self.choose()

    def accept(self, T):
        b, v = self.bufs, self.verify
        r = None if v is None else self._refiner.bufs
        _lib.call("loop_accept_kernel_wrapper", self.device, self.streams, self.num_points, self.max_loops, _p(b["found"]),
                  _p(b["match"]), _p(b["match_score"]), _p(b["frame_id"]), _p(T), _p(None if r is None else r["status"]),
                  _p(None if r is None else r["pairs"]), _p(None if r is None else r["cost"]),
                  0.0 if v is None else float(v["min_fitness"]), 0.0 if v is None else float(v["max_mean_cost"]),
                  _p(b["log_i"]), _p(b["log_T"]), _p(b["log_c"]), _p(b["nlog"]), _p(b["log_overflow"]), _p(b["accepted"]))

    def insert(self):
        b = self.bufs
        keep = self.verify is not None
        _lib.call("loop_insert_kernel_wrapper", self.device, self.streams, self.num_points, self.rings, self.sectors,
                  self.max_keyframes, _p(b["slot"]), _p(b["frame_id"]), _p(b["Dn"]), _p(b["qmask"]),
                  _p(b["cloud"]) if keep else 0, _p(b["db_desc"]), _p(b["db_mask"]), _p(b["db_frame"]),
                  _p(b["db_cloud"]) if keep else 0, _p(b["count"]))

    def search(self, trajectory=None):
        """Descriptor, score and select alone: the first three launches of a detection."""
        self.build()
        self.score(trajectory)
        self.select()

    def _body(self, trajectory):
        b = self.bufs
        self.search(trajectory)
        T = b["T0"]
        if self.verify is not None:
            self.fetch()
            start = b["T0"]
            if self.translation is not None:
                self.translate()
                start = b["T1"]
            self._refiner.register(b["staging"], b["eye"], active=b["found"], restart=b["found"])
            T = self._refiner.register(b["cloud"], start, active=b["found"])
        self.accept(T)
        self.insert()

    def refiner(self):
        """The verifying ``IcpRefiner`` (``status()``, ``diagnostics()``); None before the first call or without ``verify``."""
        return self._refiner

    def _make_refiner(self):
        """The refiner's first registration needs an active stream and a defined cloud in every row: it registers this
        call's own frames once, all active; the first verified match restarts the stream's map anyway."""
        from . import registration
        v, b = self.verify, self.bufs
        self._refiner = registration.IcpRefiner(self.streams, self.num_points, map_size=1, iters=int(v["iters"]),
                                                sigma=float(v["sigma"]), max_dist=float(v["max_dist"]), graph=False,
                                                per_stream=True)
        self._refiner.register(b["cloud"], b["eye"])

    def process(self, cloud, frame_ids, active=None, restart=None, trajectory=None, lengths=None):
        what = "ScanContextLoopDetector"
        S, n = self.streams, self.num_points
        _check_cloud(what, cloud, S, n, cuda=False)         # every argument's kind and shape first, then where it lives
        given, frame_ids = _frame_ids(what, frame_ids, S)
        if lengths is not None:
            _need(lengths, "%s: lengths" % what, torch.int32, (S,), cuda=False)
        if trajectory is not None:
            pose_stack(what, "trajectory", trajectory, S)
        act = None if active is None else stream_masks.stream_mask(active, S, "active", what)
        rst = None if restart is None else stream_masks.stream_mask(restart, S, "restart", what)
        need_cuda(cloud, given, lengths, trajectory)
        if self.bufs is None:
            self.device = cloud.device
            self._alloc()
        b = self.bufs
        stream_masks.load_words(b["active"], b["restart"], act, rst)
        b["cloud"].copy_(cloud)
        b["frame_id"].copy_(frame_ids)
        stream_masks.load_lengths(b["lengths"], lengths, n)
        if self.verify is not None and self._refiner is None:
            self._make_refiner()
        gate = trajectory is not None and self.max_distance is not None
        key = (trajectory.data_ptr(), int(trajectory.shape[0])) if gate else None
        self.replay.run(lambda: self._body(trajectory), self.device, key)


class ScanContextLoopClosure:
    """The reference's ``slam.loop_closure.LoopClosure`` interface over one stream of ``ScanContextLoopDetector``: NumPy in
    and out.  ``process_next_frame(data_dict)`` reads ``data_dict["lc_pointcloud"]`` ((m, 3) array; the first ``num_points``
    rows are used, a shorter cloud is padded with repeats of its rows and its length honoured) and ``data_dict["lc_relative_pose"]`` ((4, 4), the pose
    of this frame in the previous one; missing: the identity), and writes every closure it accepts as
    ``data_dict["se3_loop_closure_constraint_<i>_<j>"] = (T, None)``, which ``backend.GraphSLAM.next_frame`` consumes.
    ``update_positions(trajectory)`` replaces the absolute poses the position gate reads, as the reference does after an
    optimisation.  Keywords other than ``num_points``, ``max_frames``, ``device`` and ``detector`` are the detector's."""

    def __init__(self, num_points, max_frames=4096, device="cuda", detector=None, **config):
        if int(num_points) < 1 or int(max_frames) < 1:
            raise ValueError("ScanContextLoopClosure: num_points=%d and max_frames=%d must be >= 1"
                             % (int(num_points), int(max_frames)))
        self.num_points, self.max_frames, self.device = int(num_points), int(max_frames), torch.device(device)
        self.config = dict(config)
        self._detector = detector if detector is not None else ScanContextLoopDetector(1, self.num_points, device=device,
                                                                                       **self.config)
        self._traj = None
        self._last = np.eye(4)
        self._frame = 0

    @staticmethod
    def pointcloud_key():
        return "lc_pointcloud"

    @staticmethod
    def relative_pose_key():
        return "lc_relative_pose"

    def detector(self):
        return self._detector

    def init(self):
        self.clean()

    def clean(self):
        self._detector.reset()
        self._detector.poll()
        self._traj = torch.eye(4, dtype=torch.float64, device=self.device).expand(self.max_frames, 1, 4, 4).contiguous()
        self._last = np.eye(4)
        self._frame = 0

    def update_positions(self, trajectory):
        traj = np.asarray(trajectory, dtype=np.float64)
        if traj.ndim != 3 or traj.shape[1:] != (4, 4) or traj.shape[0] > self.max_frames:
            raise ValueError("ScanContextLoopClosure: trajectory must be (N <= %d, 4, 4)" % self.max_frames)
        if self._traj is None:
            raise RuntimeError("ScanContextLoopClosure: init() comes before update_positions")
        if len(traj):
            self._traj[:len(traj), 0].copy_(torch.from_numpy(np.ascontiguousarray(traj)))
            if len(traj) >= self._frame > 0:
                self._last = traj[self._frame - 1].copy()

    def process_next_frame(self, data_dict):
        from .backend import GraphSLAM
        if self._traj is None:
            raise RuntimeError("ScanContextLoopClosure: init() comes before the first frame")
        if self._frame >= self.max_frames:
            raise RuntimeError("ScanContextLoopClosure: more than max_frames=%d frames" % self.max_frames)
        if self.pointcloud_key() not in data_dict:
            return
        pc = np.asarray(data_dict[self.pointcloud_key()], dtype=np.float32)
        if pc.ndim != 2 or pc.shape[1] < 3 or pc.shape[0] < 1:
            raise ValueError("ScanContextLoopClosure: %s must be an (m >= 1, 3) array" % self.pointcloud_key())
        n = self.num_points
        m = min(n, pc.shape[0])                          # a short cloud is padded with repeats of its own rows: a repeat
        rows = np.ascontiguousarray(pc[np.arange(n) % m, :3][None], dtype=np.float32)     # changes no maximum and adds
        # no point that is not the scene's (rows of zeros would pair perfectly in the verification)
        rel = np.asarray(data_dict.get(self.relative_pose_key(), np.eye(4)), dtype=np.float64)
        if rel.shape != (4, 4):
            raise ValueError("ScanContextLoopClosure: %s must be a (4, 4) matrix" % self.relative_pose_key())
        f = self._frame
        if f > 0:
            self._last = self._last @ rel
        self._traj[f, 0].copy_(torch.from_numpy(self._last.copy()))
        self._detector.process(torch.from_numpy(rows).to(self.device), [f], trajectory=self._traj,
                               lengths=torch.tensor([m], dtype=torch.int32, device=self.device))
        self._frame = f + 1
        for r in self._detector.poll():
            data_dict[GraphSLAM.se3_loop_closure_constraint(r.i, r.j)] = (r.T, None)
