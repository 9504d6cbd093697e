"""The streams of the throughput pipelines (``graphed.PipelinedForward`` / ``PipelinedSequence``).

The HIP runtime serialises streams that share a hardware queue, and which queue a stream gets follows from the order in
which the process's streams are created and first used.  ``StreamSet`` is the native library's
stream set (include/pwclo_ops.h section 0b, csrc/pipeline.hip): all streams made and first used back to back inside one
call, wrapped as ``torch.cuda.ExternalStream`` for the rest of the package.

``PWCLO_PIPE_STREAMS`` (read once per process): ``native`` (default) = the set above; ``torch`` = streams from torch's
pool, as before the set existed -- the A/B switch.
"""
import ctypes
import os
import sys

import torch

from . import _lib

MAX_STREAMS = 8          # PWCLO_STREAM_SET_MAX
_EINVAL = 10001          # PWCLO_EINVAL

_mode = None
_deferred = []           # handles whose owner died while a graph was being captured: destroyed at the next safe point


def parse_mode(value):
    """``PWCLO_PIPE_STREAMS`` value (None = unset) -> ``"native"`` or ``"torch"``; anything else is an error."""
    v = (value or "").strip().lower()
    if v in ("", "native"):
        return "native"
    if v == "torch":
        return "torch"
    raise ValueError("PWCLO_PIPE_STREAMS=%r: expected 'native' or 'torch'" % (value,))


def mode():
    """The process's choice: the environment is read at the first call and never again."""
    global _mode
    if _mode is None:
        _mode = parse_mode(os.environ.get("PWCLO_PIPE_STREAMS"))
    return _mode


def lanes(depth):
    """How many streams a pipeline of ``depth`` slots rotates its calls over when the streams are native ones.

    The runtime multiplexes the process's streams onto its hardware queues (``hw_queues()``; the runtime's default is 4)
    and one queue's worth is taken by the rest of the process -- the null stream, torch's side and capture streams, the
    communicator's: measured on MI355X, with 4 queues three replays run side by side and a fourth stream, wherever it is
    created, shares a queue with one of the three and serialises with it.  So with more queues than
    slots every slot has its stream; otherwise queues - 1 streams carry all slots in turn."""
    from . import hw_queues
    q = hw_queues() or 4
    return depth if q > depth else max(1, min(depth, q - 1))


def _check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed (error %d%s)" % (what, rc, ": invalid argument or handle" if rc == _EINVAL else ""))


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing()


def _drain_deferred():
    if _deferred and not _capturing():
        lib = _lib.load()
        while _deferred:
            lib.pwclo_stream_set_destroy(_deferred.pop())


class SlotEvent:
    """Completion of one slot of a ``StreamSet`` (what ``PipelinedForward.events`` holds on the native path)."""

    def __init__(self, owner, slot):
        self.owner, self.slot = owner, slot

    def query(self):
        return self.owner.query(self.slot)

    def synchronize(self):
        self.owner.synchronize_slot(self.slot)


class StreamSet:
    """``n`` streams of the native set on ``device``; ``wrap(i)`` hands stream i out as a ``torch.cuda.ExternalStream``.
    The wrappers keep the set alive (a second pipeline may go on using them after the first is gone); the set is
    destroyed, after a device sync, when the last reference goes -- put off to the next safe point if that happens while
    a graph is being captured."""

    def __init__(self, n, device):
        self._handle = 0
        self._lib = lib = _lib.load()
        _drain_deferred()
        if _capturing():
            raise RuntimeError("a pipeline's stream set cannot be created during graph capture")
        device = torch.device(device)
        h = ctypes.c_longlong(0)
        with torch.cuda.device(device):
            _check(lib.pwclo_stream_set_create(int(n), ctypes.byref(h)), "pwclo_stream_set_create(%d)" % n)
        self._handle, self.n, self.device, self.max_slots = h.value, int(n), device, MAX_STREAMS

    def wrap(self, i):
        """Stream i as a new ``torch.cuda.ExternalStream`` that keeps this set alive (the set holds no wrapper: no cycle,
        so the set goes when its pipeline and the last wrapper have gone, not when the collector next runs)."""
        st = torch.cuda.ExternalStream(self.handle(i), device=self.device)
        st._pwclo_set, st._pwclo_index = self, i
        return st

    def handle(self, i):
        """hipStream_t of stream i as an integer."""
        p = ctypes.c_void_p()
        _check(self._lib.pwclo_stream_set_stream(self._handle, i, ctypes.byref(p)), "pwclo_stream_set_stream")
        return p.value

    def wait_stream(self, i, other):
        """Stream i waits for what is queued on ``other`` (a torch stream) now."""
        _check(self._lib.pwclo_stream_set_wait_stream(self._handle, i, ctypes.c_void_p(other.cuda_stream)),
               "pwclo_stream_set_wait_stream")

    def record(self, slot, i):
        _check(self._lib.pwclo_stream_set_record(self._handle, slot, i), "pwclo_stream_set_record")
        return SlotEvent(self, slot)

    def query(self, slot):
        rc = self._lib.pwclo_stream_set_query(self._handle, slot)
        if rc < 0:
            _check(-rc, "pwclo_stream_set_query")
        return rc == 1

    def wait_slot(self, slot, stream):
        """``stream`` (a torch stream) waits for the slot's completion."""
        _check(self._lib.pwclo_stream_set_wait_slot(self._handle, slot, ctypes.c_void_p(stream.cuda_stream)),
               "pwclo_stream_set_wait_slot")

    def synchronize_slot(self, slot):
        _check(self._lib.pwclo_stream_set_synchronize_slot(self._handle, slot), "pwclo_stream_set_synchronize_slot")

    def synchronize(self):
        _check(self._lib.pwclo_stream_set_synchronize(self._handle), "pwclo_stream_set_synchronize")

    def close(self):
        """Destroy the set now (device sync first).  Its stream wrappers must not be used afterwards."""
        h, self._handle = self._handle, 0
        if h:
            if _capturing():
                _deferred.append(h)
            else:
                _check(self._lib.pwclo_stream_set_destroy(h), "pwclo_stream_set_destroy")

    def __del__(self):
        if getattr(self, "_handle", 0) and not sys.is_finalizing():
            try:
                self.close()
            except Exception:       # a destructor has nobody to raise to
                pass
