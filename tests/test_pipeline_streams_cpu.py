"""The pipelines' stream set without a GPU: what the C ABI (include/pwclo_ops.h section 0b, csrc/pipeline.hip) refuses, it
refuses with an error code before any HIP call -- so these calls return on a machine without a device -- and how
``PWCLO_PIPE_STREAMS`` is parsed."""
import ctypes
import os
import re

import pytest

from pwclonet_pylidarslam_amd import _lib, pipe_streams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 10001
NAMES = ["pwclo_stream_set_create", "pwclo_stream_set_size", "pwclo_stream_set_stream", "pwclo_stream_set_wait_stream",
         "pwclo_stream_set_record", "pwclo_stream_set_query", "pwclo_stream_set_wait_slot",
         "pwclo_stream_set_synchronize_slot", "pwclo_stream_set_synchronize", "pwclo_stream_set_destroy"]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_header_declares_what_the_binding_declares(lib):
    with open(os.path.join(ROOT, "include", "pwclo_ops.h")) as f:
        header = f.read()
    for name in NAMES:
        m = re.search(r"\bint %s\(([^)]*)\);" % name, header)
        assert m is not None, "%s is not declared in include/pwclo_ops.h" % name
        args, res = _lib.SIGNATURES[name]
        assert len(m.group(1).split(",")) == len(args) and res is ctypes.c_int, name
        assert hasattr(lib, name)
    assert "#define PWCLO_STREAM_SET_MAX %d" % pipe_streams.MAX_STREAMS in header
    assert "#define PWCLO_EINVAL %d" % EINVAL in header
    assert lib.pwclo_abi_version() == 1                      # additions only


@pytest.mark.parametrize("n", [0, 9, -1, 1 << 20])
def test_create_refuses_a_stream_count_outside_1_to_8(lib, n):
    h = ctypes.c_longlong(77)
    assert lib.pwclo_stream_set_create(n, ctypes.byref(h)) == EINVAL
    assert h.value == 0                                      # no handle is handed out with a refusal
    assert lib.pwclo_stream_set_create(4, None) == EINVAL    # nowhere to put the handle: refused before anything is made


@pytest.mark.parametrize("handle", [0, -3, 1 << 40])
def test_a_handle_that_is_not_live_is_refused_everywhere(lib, handle):
    """Ids are handed out from 1 upwards and never reused, so 0, a negative and a far-off id stand for a destroyed set."""
    p = ctypes.c_void_p(5)
    assert lib.pwclo_stream_set_size(handle) == -EINVAL
    assert lib.pwclo_stream_set_stream(handle, 0, ctypes.byref(p)) == EINVAL and p.value is None
    assert lib.pwclo_stream_set_wait_stream(handle, 0, None) == EINVAL
    assert lib.pwclo_stream_set_record(handle, 0, 0) == EINVAL
    assert lib.pwclo_stream_set_query(handle, 0) == -EINVAL
    assert lib.pwclo_stream_set_wait_slot(handle, 0, None) == EINVAL
    assert lib.pwclo_stream_set_synchronize_slot(handle, 0) == EINVAL
    assert lib.pwclo_stream_set_synchronize(handle) == EINVAL
    assert lib.pwclo_stream_set_destroy(handle) == EINVAL
    assert lib.pwclo_last_error() == 0                       # the sticky launch status is not involved


@pytest.mark.parametrize("index", [-1, 8, 1 << 30])
def test_an_index_out_of_range_is_refused(lib, index):
    p = ctypes.c_void_p()
    for handle in (0, 1):
        assert lib.pwclo_stream_set_stream(handle, index, ctypes.byref(p)) == EINVAL
        assert lib.pwclo_stream_set_wait_stream(handle, index, None) == EINVAL
        assert lib.pwclo_stream_set_record(handle, index, 0) == EINVAL
        assert lib.pwclo_stream_set_record(handle, 0, index) == EINVAL
        assert lib.pwclo_stream_set_query(handle, index) == -EINVAL
        assert lib.pwclo_stream_set_wait_slot(handle, index, None) == EINVAL
        assert lib.pwclo_stream_set_synchronize_slot(handle, index) == EINVAL
    assert lib.pwclo_stream_set_stream(0, 0, None) == EINVAL


@pytest.mark.parametrize("value, want", [(None, "native"), ("", "native"), ("native", "native"), ("torch", "torch"),
                                         (" Torch ", "torch"), ("NATIVE", "native")])
def test_pipe_streams_values(value, want):
    assert pipe_streams.parse_mode(value) == want


@pytest.mark.parametrize("value", ["0", "1", "hip", "torch,native"])
def test_pipe_streams_refuses_anything_else(value):
    with pytest.raises(ValueError, match="PWCLO_PIPE_STREAMS"):
        pipe_streams.parse_mode(value)


def test_pipe_streams_is_read_once_per_process(monkeypatch):
    monkeypatch.setattr(pipe_streams, "_mode", None)
    monkeypatch.setenv("PWCLO_PIPE_STREAMS", "torch")
    assert pipe_streams.mode() == "torch"
    monkeypatch.setenv("PWCLO_PIPE_STREAMS", "native")
    assert pipe_streams.mode() == "torch"                    # the first read stands
    monkeypatch.setattr(pipe_streams, "_mode", None)         # (monkeypatch restores the process's own value afterwards)
    monkeypatch.delenv("PWCLO_PIPE_STREAMS")
    assert pipe_streams.mode() == "native"


@pytest.mark.parametrize("queues, depth, want", [(None, 4, 3), ("4", 4, 3), ("8", 4, 4), ("4", 3, 3), ("4", 1, 1), ("5", 4, 4),
                                                 ("8", 8, 7), ("2", 4, 1), ("1", 4, 1), ("32", 6, 6)])
def test_lanes_follow_the_queue_count_the_process_asked_for(monkeypatch, queues, depth, want):
    """More queues than slots: a stream per slot; otherwise queues - 1 streams (one queue's worth goes to the rest of the
    process), never fewer than one.  Unset = the runtime's default of 4."""
    if queues is None:
        monkeypatch.delenv("GPU_MAX_HW_QUEUES", raising=False)
    else:
        monkeypatch.setenv("GPU_MAX_HW_QUEUES", queues)
    assert pipe_streams.lanes(depth) == want
