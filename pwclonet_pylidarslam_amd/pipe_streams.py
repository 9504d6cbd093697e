"""The streams of the throughput pipelines (``graphed.PipelinedForward`` / ``PipelinedSequence``).

The HIP runtime serialises streams that share a hardware queue, and which queue a stream gets follows from the order in
which the process's streams are created and first used.  ``StreamSet`` is the native library's
stream set (include/pwclo_ops.h section 0b, csrc/pipeline.hip): all streams made and first used back to back inside one
call, wrapped as ``torch.cuda.ExternalStream`` for the rest of the package.

``PWCLO_PIPE_STREAMS`` (read once per process): ``native`` (default) = the set above; ``torch`` = streams from torch's
pool, as before the set existed -- the A/B switch.

``PWCLO_PIPE_PRIORITY`` (read once per process): the priority class of the set's streams, ``normal`` | ``high`` | ``low`` |
``mixed`` | ``auto`` -- the layouts of ``pwclo_stream_set_create_ex``.  The runtime keeps its hardware queues per
priority class; ``auto`` keeps the first layout in which the set's probe finds every stream running side by side.

Every set measures, in its create call, how many of its streams run side by side (``StreamSet.side_by_side``,
``StreamSet.together``).  With a layout chosen -- by the variable, or ``auto`` for a program that called
``configure_hw_queues()`` -- a pipeline rotates over those (``rotation``), not over a number derived from the queue count.
A process that chose nothing (``priority() == FORMULA``) keeps normal streams and the queue-count formula ``lanes``.
"""
import ctypes
import os
import sys

import torch

from . import _lib

MAX_STREAMS = 8          # PWCLO_STREAM_SET_MAX
_EINVAL = 10001          # PWCLO_EINVAL

LAYOUTS = {"auto": -1, "normal": 0, "high": 1, "low": 2, "mixed": 3}     # PWCLO_STREAM_LAYOUT_*
_LAYOUT_NAMES = {v: k for k, v in LAYOUTS.items()}

_mode = None
_priority = None
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


def parse_priority(value):
    """``PWCLO_PIPE_PRIORITY`` value -> a key of ``LAYOUTS``, None when unset or empty; anything else is an error."""
    v = (value or "").strip().lower()
    if v == "":
        return None
    if v in LAYOUTS:
        return v
    raise ValueError("PWCLO_PIPE_PRIORITY=%r: expected 'normal', 'high', 'low', 'mixed' or 'auto'" % (value,))


FORMULA = "formula"      # priority() of a process that asked for nothing: normal streams, lanes(depth) of them


def default_priority(requested_queues):
    """What an unset ``PWCLO_PIPE_PRIORITY`` means.  A program that called ``configure_hw_queues()`` (``requested_queues``
    is what it passed) asked for pipelines as deep as they go: ``auto``.  One that never did (None) gets what it got
    before the layouts existed -- normal-priority streams only, rotated by the queue-count formula ``lanes``: a library
    does not put a host process's streams into another priority class unasked."""
    return "auto" if requested_queues is not None else FORMULA


def priority():
    """The process's choice -- a key of ``LAYOUTS``, or ``FORMULA``: the environment (and whether the program called
    ``configure_hw_queues()``) is read at the first call and never again."""
    global _priority
    if _priority is None:
        from . import requested_hw_queues
        _priority = parse_priority(os.environ.get("PWCLO_PIPE_PRIORITY")) or default_priority(requested_hw_queues())
    return _priority


def rotation(depth, side_by_side, together=None):
    """(lanes, stream indices) of a pipeline of ``depth`` slots on a set whose probe found ``side_by_side`` streams running
    together, ``together`` being their indices in rising order (None: the first ``side_by_side``).  The calls rotate over
    min(depth, side_by_side) streams, the first that many of ``together``: call c goes to stream indices[c % lanes]."""
    if depth < 1 or side_by_side < 1:
        raise ValueError("rotation(%r, %r): both must be at least 1" % (depth, side_by_side))
    together = tuple(range(side_by_side)) if together is None else tuple(together)
    if len(together) != side_by_side or list(together) != sorted(set(together)) or together[0] < 0:
        raise ValueError("rotation: %r are not %d distinct stream indices in rising order" % (together, side_by_side))
    n = min(depth, side_by_side)
    return n, together[:n]


def lanes(depth):
    """How many native streams a pipeline of ``depth`` slots rotates its calls over in a process that chose no layout
    (``priority() == FORMULA``); where one was chosen the set's own measurement decides, through ``rotation``.

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
    a graph is being captured.

    ``side_by_side``, ``together``, ``layout``, ``probe_ns``: what the create call measured (how many of the streams ran
    side by side, which, in which layout -- the one ``auto`` kept, or ``normal`` on a device with one priority level --
    and how long the probe's longest launch took)."""

    def __init__(self, n, device, layout=None):
        """``layout``: a key of ``LAYOUTS``; None = the process's ``priority()`` (normal where that is ``FORMULA``)."""
        self._handle = 0
        self._lib = lib = _lib.load()
        _drain_deferred()
        if _capturing():
            raise RuntimeError("a pipeline's stream set cannot be created during graph capture")
        device = torch.device(device)
        asked = priority() if layout is None else layout
        # a set made for a process that chose no layout is a normal one whose pipelines keep the queue-count formula
        self.follows_probe = asked != FORMULA
        if asked == FORMULA:
            asked = "normal"
        h = ctypes.c_longlong(0)
        with torch.cuda.device(device):
            _check(lib.pwclo_stream_set_create_ex(int(n), LAYOUTS[asked], ctypes.byref(h)),
                   "pwclo_stream_set_create_ex(%d, %s)" % (n, asked))
        self._handle, self.n, self.device, self.max_slots = h.value, int(n), device, MAX_STREAMS
        # what the create call measured: how many streams ran side by side, which, in which layout, how long a probe ran
        k, lay, mask, ns = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_uint(0), ctypes.c_longlong(0)
        _check(lib.pwclo_stream_set_concurrency(h.value, ctypes.byref(k)), "pwclo_stream_set_concurrency")
        _check(lib.pwclo_stream_set_probe(h.value, ctypes.byref(lay), ctypes.byref(mask), ctypes.byref(ns)),
               "pwclo_stream_set_probe")
        self.side_by_side, self.layout, self.probe_ns = k.value, _LAYOUT_NAMES[lay.value], ns.value
        self.together = tuple(i for i in range(self.n) if mask.value >> i & 1)

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
