"""The stream set's priority layouts and probe without a GPU: how ``PWCLO_PIPE_PRIORITY`` is parsed, the pure mapping from
a probe result to the lanes and stream indices a pipeline rotates over, and what the new entry points of the C ABI
(include/pwclo_ops.h section 0b) refuse before any HIP call."""
import ctypes
import os
import re

import pytest

import pwclonet_pylidarslam_amd
from pwclonet_pylidarslam_amd import _lib, pipe_streams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 10001


@pytest.mark.parametrize("value, want", [(None, None), ("", None), ("  ", None), ("auto", "auto"), ("normal", "normal"),
                                         ("high", "high"), ("low", "low"), ("mixed", "mixed"), (" High ", "high"),
                                         ("MIXED", "mixed")])
def test_pipe_priority_values(value, want):
    assert pipe_streams.parse_priority(value) == want


@pytest.mark.parametrize("value", ["0", "1", "-1", "highest", "normal,high", "hi", "none"])
def test_pipe_priority_refuses_anything_else(value):
    with pytest.raises(ValueError, match="PWCLO_PIPE_PRIORITY"):
        pipe_streams.parse_priority(value)


def test_pipe_priority_is_read_once_per_process(monkeypatch):
    monkeypatch.setattr(pipe_streams, "_priority", None)
    monkeypatch.setenv("PWCLO_PIPE_PRIORITY", "low")
    assert pipe_streams.priority() == "low"
    monkeypatch.setenv("PWCLO_PIPE_PRIORITY", "high")
    assert pipe_streams.priority() == "low"                  # the first read stands
    monkeypatch.setenv("PWCLO_PIPE_PRIORITY", "nonsense")
    assert pipe_streams.priority() == "low"                  # ... and the variable is not even parsed again
    monkeypatch.setattr(pipe_streams, "_priority", None)     # (monkeypatch restores the process's own value afterwards)
    with pytest.raises(ValueError, match="PWCLO_PIPE_PRIORITY"):
        pipe_streams.priority()
    monkeypatch.delenv("PWCLO_PIPE_PRIORITY")
    monkeypatch.setattr(pwclonet_pylidarslam_amd, "_requested", 8)
    assert pipe_streams.priority() == "auto"                 # unset, in a program that called configure_hw_queues()


def test_unset_means_auto_only_for_a_program_that_called_configure_hw_queues(monkeypatch):
    """A process that asked for nothing keeps normal streams and the queue-count formula; ``configure_hw_queues()`` --
    granted or not -- is how a program asks for pipelines as deep as they go; the variable always wins."""
    assert pipe_streams.default_priority(None) == pipe_streams.FORMULA
    assert pipe_streams.default_priority(8) == pipe_streams.default_priority(1) == "auto"
    assert pipe_streams.FORMULA not in pipe_streams.LAYOUTS
    monkeypatch.delenv("PWCLO_PIPE_PRIORITY", raising=False)
    monkeypatch.setattr(pwclonet_pylidarslam_amd, "_requested", None)
    monkeypatch.setattr(pipe_streams, "_priority", None)
    assert pipe_streams.priority() == pipe_streams.FORMULA
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", "4")             # the environment keeps the count down: asked, not granted
    assert pwclonet_pylidarslam_amd.configure_hw_queues(8) == 4
    assert pwclonet_pylidarslam_amd.requested_hw_queues() == 8 and pwclonet_pylidarslam_amd.hw_queues() == 4
    assert pipe_streams.priority() == pipe_streams.FORMULA   # read once: the first answer stands
    monkeypatch.setattr(pipe_streams, "_priority", None)
    assert pipe_streams.priority() == "auto"
    monkeypatch.setattr(pipe_streams, "_priority", None)
    monkeypatch.setenv("PWCLO_PIPE_PRIORITY", "normal")
    assert pipe_streams.priority() == "normal"
    monkeypatch.setattr(pwclonet_pylidarslam_amd, "_requested", None)
    monkeypatch.setattr(pipe_streams, "_priority", None)
    monkeypatch.setenv("PWCLO_PIPE_PRIORITY", "auto")
    assert pipe_streams.priority() == "auto"


def test_layout_numbers_are_the_headers():
    with open(os.path.join(ROOT, "include", "pwclo_ops.h")) as f:
        header = f.read()
    for name, value in pipe_streams.LAYOUTS.items():
        m = re.search(r"#define PWCLO_STREAM_LAYOUT_%s \(?(-?\d+)\)?" % name.upper(), header)
        assert m is not None and int(m.group(1)) == value, name
    assert sorted(pipe_streams.LAYOUTS.values()) == [-1, 0, 1, 2, 3]


@pytest.mark.parametrize("depth", range(1, 9))
@pytest.mark.parametrize("side_by_side", range(1, 9))
def test_rotation_is_the_first_min_depth_side_by_side_streams_that_ran_together(depth, side_by_side):
    n, idx = pipe_streams.rotation(depth, side_by_side)
    assert n == min(depth, side_by_side) and idx == tuple(range(n))
    # the streams that ran together need not be the first ones of the set: the indices are taken from them, in order
    together = tuple(range(8 - side_by_side, 8))
    n2, idx2 = pipe_streams.rotation(depth, side_by_side, together)
    assert n2 == n and idx2 == together[:n] and len(set(idx2)) == n
    gaps = tuple(sorted((3 * i + 1) % 8 for i in range(side_by_side)))      # 1, 4, 7, 2, 5, 0, 3, 6 sorted: with holes
    assert pipe_streams.rotation(depth, side_by_side, gaps) == (n, gaps[:n])
    # call c goes to indices[c % lanes]: over 2 * depth + 1 calls every lane is used and no other stream is
    used = {idx2[c % n2] for c in range(2 * depth + 1)}
    assert used == set(idx2)


@pytest.mark.parametrize("args", [(0, 1), (1, 0), (4, 3, (0, 1)), (4, 2, (1, 1)), (4, 2, (2, 1)), (4, 1, (-1,))])
def test_rotation_refuses_what_no_probe_reports(args):
    with pytest.raises(ValueError):
        pipe_streams.rotation(*args)


def test_rotation_does_not_look_at_the_queue_count(monkeypatch):
    """``lanes(depth)`` stays the formula of the queue count; ``rotation`` is the measurement's and ignores it."""
    for q in ("1", "4", "8"):
        monkeypatch.setenv("GPU_MAX_HW_QUEUES", q)
        assert pipe_streams.rotation(4, 4) == (4, (0, 1, 2, 3))
        assert pipe_streams.rotation(4, 2, (1, 3)) == (2, (1, 3))
    assert pipe_streams.lanes(4) == 4
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", "4")
    assert pipe_streams.lanes(4) == 3


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_header_declares_the_new_entry_points(lib):
    with open(os.path.join(ROOT, "include", "pwclo_ops.h")) as f:
        header = f.read()
    for name in ("pwclo_stream_set_create_ex", "pwclo_stream_set_concurrency", "pwclo_stream_set_probe"):
        m = re.search(r"\bint %s\(([^)]*)\);" % name, header)
        assert m is not None, "%s is not declared in include/pwclo_ops.h" % name
        args, res = _lib.SIGNATURES[name]
        assert len(m.group(1).split(",")) == len(args) and res is ctypes.c_int, name
        assert hasattr(lib, name)


@pytest.mark.parametrize("n, layout", [(0, 0), (9, 0), (-1, 1), (4, 4), (4, -2), (4, 1 << 20), (1, 99)])
def test_create_ex_refuses_a_count_or_layout_it_does_not_know(lib, n, layout):
    h = ctypes.c_longlong(77)
    assert lib.pwclo_stream_set_create_ex(n, layout, ctypes.byref(h)) == EINVAL
    assert h.value == 0                                      # no handle is handed out with a refusal
    assert lib.pwclo_stream_set_create_ex(4, 0, None) == EINVAL
    assert lib.pwclo_last_error() == 0


@pytest.mark.parametrize("handle", [0, -3, 1 << 40])
def test_the_probe_readers_refuse_a_handle_that_is_not_live(lib, handle):
    k, lay, mask, ns = ctypes.c_int(5), ctypes.c_int(5), ctypes.c_uint(5), ctypes.c_longlong(5)
    assert lib.pwclo_stream_set_concurrency(handle, ctypes.byref(k)) == EINVAL and k.value == 0
    assert lib.pwclo_stream_set_probe(handle, ctypes.byref(lay), ctypes.byref(mask), ctypes.byref(ns)) == EINVAL
    assert (lay.value, mask.value, ns.value) == (0, 0, 0)
    assert lib.pwclo_stream_set_concurrency(handle, None) == EINVAL
    assert lib.pwclo_stream_set_probe(handle, None, ctypes.byref(mask), ctypes.byref(ns)) == EINVAL
    assert lib.pwclo_stream_set_probe(handle, ctypes.byref(lay), None, ctypes.byref(ns)) == EINVAL
    assert lib.pwclo_stream_set_probe(handle, ctypes.byref(lay), ctypes.byref(mask), None) == EINVAL
