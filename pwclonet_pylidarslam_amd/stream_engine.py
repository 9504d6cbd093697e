"""What the per-stream device modules (the three refiners, ``PoseGraph``, ``ScanContextLoopDetector``, ``GlobalMap``) share
in front of their kernels: the replay protocol of their public calls and the vocabulary of their
argument checks.  Every check raises before anything is launched, with the caller's prefix in front."""
import numpy as np
import torch

from . import _lib


# ---- replay ------------------------------------------------------------------------------------------------------------

class Replay:
    """The replay protocol of a public call: ``run(body, device, key)`` calls ``body()`` on call 0
    and wherever ``graph`` is false; a later call captures ``body()`` once per key, after a device sync, and replays it.
    ``calls``: completed runs; ``captures``: graphs captured so far, which ``drop()`` keeps; ``graphs``: key -> graph.  A
    body that raises leaves all three as they were."""

    def __init__(self, graph):
        self.enabled, self.calls, self.captures, self.graphs = bool(graph), 0, 0, {}

    def graph(self, key=None):
        return self.graphs.get(key)

    def run(self, body, device, key=None):
        if not self.enabled or self.calls == 0:
            body()
        else:
            g = self.graphs.get(key)
            if g is None:
                torch.cuda.synchronize(device)
                g = torch.cuda.CUDAGraph()
                with _lib.capture(g):
                    body()
                self.graphs[key] = g
                self.captures += 1
            g.replay()
        self.calls += 1

    def drop(self):
        """Forget every captured graph: their launches hold settings that no longer apply."""
        self.graphs.clear()


class Replayed:
    """Base of a class that runs its public call through ``self.replay``: the counters under their public names."""
    calls = property(lambda self: self.replay.calls)
    captures = property(lambda self: self.replay.captures)


# ---- arguments ---------------------------------------------------------------------------------------------------------

def ptr(t):
    return t.data_ptr() if t is not None else 0


def need_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("CPU not supported")


def need(t, name, dtype, shape=None, cuda=True):
    """ValueError for the wrong kind or shape, then (``cuda``) RuntimeError for a host tensor, then ValueError for a layout
    that is not contiguous.  ``cuda=False`` leaves the question where the tensor lives to a later ``need_cuda``."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError("%s must be a %s tensor%s, got %s %s" % (
            name, str(dtype).replace("torch.", ""), "" if shape is None else " of shape %s" % (tuple(shape),),
            getattr(t, "dtype", type(t)), tuple(getattr(t, "shape", ()))))
    if cuda:
        need_cuda(t)
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)


def stream_count(what, streams, limit):
    S = int(streams)
    if not 1 <= S <= limit:
        raise ValueError("%s: streams=%d outside [1, %d]" % (what, S, limit))
    return S


def stream_index(owner, what, stream, S):
    """A host stream index -> int in [0, S); the message starts with ``owner`` and ``what``, either of which may be None."""
    s = int(stream)
    if not 0 <= s < S:
        raise ValueError("%s: stream=%d outside [0, %d)" % (": ".join(w for w in (owner, what) if w), s, S))
    return s


def stream_indices(owner, what, streams, S):
    """``streams=`` of a reset: host indices, or None for all."""
    return range(S) if streams is None else [stream_index(owner, what, s, S) for s in streams]


def frame_ids(what, frame_ids, S):
    """(S,) int32 tensor or host integers -> (the caller's tensor or None, the (S,) int32 tensor to copy from): a host
    sequence may stay on the host."""
    if isinstance(frame_ids, torch.Tensor):
        need(frame_ids, "%s: frame_ids" % what, torch.int32, (S,), cuda=False)
        return frame_ids, frame_ids
    ids = np.asarray(frame_ids)
    if ids.shape != (S,) or ids.dtype.kind not in "iu" or ids.min() < 0:
        raise ValueError("%s: frame_ids must be (%d,) non-negative integers" % (what, S))
    return None, torch.from_numpy(ids.astype(np.int32))


def pose_stack(what, name, t, S):
    """A buffer of absolute poses read by frame id: fp64 (frames >= 1, S, 4, 4), contiguous."""
    if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[0] < 1:
        raise ValueError("%s: %s must be float64 (frames >= 1, %d, 4, 4)" % (what, name, S))
    need(t, "%s: %s" % (what, name), torch.float64, (t.shape[0], S, 4, 4), cuda=False)


def init_poses(what, init, S):
    """The initial guess of a refiner: fp64 (S, 4, 4) transforms or fp32 (S, 7) pose rows."""
    if not isinstance(init, torch.Tensor) or (init.dtype, tuple(init.shape)) not in (
            (torch.float64, (S, 4, 4)), (torch.float32, (S, 7))):
        raise ValueError("%s: init must be float64 (%d, 4, 4) or float32 (%d, 7) pose rows, got %s %s"
                         % (what, S, S, getattr(init, "dtype", type(init)), tuple(getattr(init, "shape", ()))))


# ---- the solver settings of the refiners' constructors, in the order they check them ----------------------------------

def need_iters(what, iters):
    if int(iters) < 1:
        raise ValueError("%s: iters=%d must be >= 1" % (what, int(iters)))


def need_sigma(what, sigma):
    if not float(sigma) > 0.0 or not np.isfinite(float(sigma)):
        raise ValueError("%s: sigma=%r must be finite and > 0" % (what, sigma))


def need_max_dist(what, max_dist):
    if not float(max_dist) >= 0.0:
        raise ValueError("%s: max_dist=%r must be >= 0" % (what, max_dist))


def need_solver(what, damping, threshold_delta_pose, min_pairs):
    if not float(damping) >= 0.0 or not np.isfinite(float(damping)):
        raise ValueError("%s: damping=%r must be finite and >= 0" % (what, damping))
    if not float(threshold_delta_pose) >= 0.0:
        raise ValueError("%s: threshold_delta_pose=%r must be >= 0" % (what, threshold_delta_pose))
    if int(min_pairs) < 1:
        raise ValueError("%s: min_pairs=%d must be >= 1 (an empty map freezes a stream through it)" % (what, int(min_pairs)))
