"""The stream set's probe and priority layouts on the GPU (csrc/pipeline.hip, include/pwclo_ops.h section 0b):

* the probe: a set of 1 reports 1 stream side by side, a set of 2 reports 2, a set of n never more than n, and the create
  call -- which runs the probe -- returns within 20 x the probe's measured launch length x n (the launch is a fixed number
  of rounds of an ALU chain sized to about 0.5 ms: it ends by itself);
* the layouts: each creates and destroys cleanly at n = 4, an unknown one is refused, a destroyed handle is refused;
* the pipeline: under every ``PWCLO_PIPE_PRIORITY`` value (one fresh child process each: the variable is read once)
  ``PipelinedForward`` at depth 4 gives, over 9 calls on 9 inputs, byte for byte the poses of a serial ``GraphedForward``;
* ``auto``: the layout a pipeline reports is one whose probe value is the lane count it uses;
* a process that chose no layout (no variable, no ``configure_hw_queues()``) keeps normal streams and ``lanes(depth)``.
"""
import ctypes
import json
import os
import subprocess
import sys
import time

import pytest
import torch

import pipe_priority_cases as T
from pwclonet_pylidarslam_amd import _lib, pipe_streams

pytestmark = pytest.mark.gpu

EINVAL = 10001
LAYOUT_NUMBERS = sorted(pipe_streams.LAYOUTS.values())          # auto, normal, high, low, mixed


def _create(lib, n, layout):
    """-> (return code, handle, seconds the create call took)"""
    h = ctypes.c_longlong(0)
    t0 = time.perf_counter()
    rc = lib.pwclo_stream_set_create_ex(n, layout, ctypes.byref(h))
    return rc, h.value, time.perf_counter() - t0


def _probe(lib, handle):
    """-> (side_by_side, layout, indices that ran together, longest probe launch in seconds)"""
    k, lay, mask, ns = ctypes.c_int(-1), ctypes.c_int(-9), ctypes.c_uint(0), ctypes.c_longlong(0)
    assert lib.pwclo_stream_set_concurrency(handle, ctypes.byref(k)) == 0
    assert lib.pwclo_stream_set_probe(handle, ctypes.byref(lay), ctypes.byref(mask), ctypes.byref(ns)) == 0
    return k.value, lay.value, [i for i in range(32) if mask.value >> i & 1], ns.value * 1e-9


@pytest.fixture(scope="module")
def lib(cuda):
    """The library with its code object loaded and the device's queues in use: one set made and destroyed, so that the
    timed create calls below measure the create call and not the process's first launch."""
    lib = _lib.load()
    with torch.cuda.device(cuda):
        torch.zeros(1, device=cuda)
        rc, h, _ = _create(lib, 4, 0)
        assert rc == 0 and lib.pwclo_stream_set_destroy(h) == 0
    return lib


@pytest.mark.parametrize("n", [1, 2, 3, 4, 8])
def test_probe_counts_the_streams_that_run_side_by_side_and_ends_by_itself(lib, cuda, n):
    with torch.cuda.device(cuda):
        rc, h, seconds = _create(lib, n, 0)
    assert rc == 0 and h > 0
    try:
        k, layout, together, launch = _probe(lib, h)
        print("n=%d: side_by_side=%d together=%s probe launch %.1f us, create call %.2f ms"
              % (n, k, together, launch * 1e6, seconds * 1e3))
        assert layout == 0
        assert 1 <= k <= n                                      # never more than the set has streams
        assert len(together) == k and all(i < n for i in together)
        if n <= 2:                                              # two free queues exist in every configuration
            assert k == n
        # sized to about 0.5 ms by the calibration launch (the clocks may move between the two: within a factor of 4)
        assert 0.125e-3 < launch < 2e-3
        assert seconds < 20 * launch * n                        # the probe's kernel ended by itself, and soon
    finally:
        assert lib.pwclo_stream_set_destroy(h) == 0


def test_stream_set_exports_what_the_probe_measured(lib, cuda):
    s = pipe_streams.StreamSet(2, cuda, layout="normal")
    try:
        assert s.side_by_side == 2 and s.together == (0, 1) and s.layout == "normal" and s.probe_ns > 0
        assert _probe(lib, s._handle)[0] == s.side_by_side
    finally:
        s.close()


@pytest.mark.parametrize("layout", LAYOUT_NUMBERS)
def test_every_layout_creates_and_destroys_cleanly(lib, cuda, layout):
    with torch.cuda.device(cuda):
        rc, h, _ = _create(lib, 4, layout)
    assert rc == 0 and h > 0
    k, got, together, _ = _probe(lib, h)
    print("layout %d -> layout %d, side_by_side %d, together %s" % (layout, got, k, together))
    assert 1 <= k <= 4 and len(together) == k
    assert got in (layout, 0) if layout >= 0 else got in (0, 1, 2, 3)   # 0: one priority level, or auto's fall-back
    if layout < 0 and got != 0:
        assert k == 4                                           # auto leaves normal only for a layout that reaches n
    p, handles = ctypes.c_void_p(), set()
    for i in range(4):
        assert lib.pwclo_stream_set_stream(h, i, ctypes.byref(p)) == 0 and p.value
        handles.add(p.value)
    assert len(handles) == 4 and lib.pwclo_stream_set_size(h) == 4
    x = torch.zeros(256, device=cuda)
    torch.cuda.synchronize(cuda)
    with torch.cuda.stream(torch.cuda.ExternalStream(p.value, device=cuda)):    # the last stream carries work
        y = x + 3
    assert lib.pwclo_stream_set_synchronize(h) == 0 and float(y.sum()) == 768.0
    assert lib.pwclo_stream_set_destroy(h) == 0
    assert lib.pwclo_stream_set_size(h) == -EINVAL
    assert lib.pwclo_last_error() == 0


def test_unknown_layout_and_destroyed_handle_are_refused(lib, cuda):
    for layout in (4, -2, 17):
        rc, h, _ = _create(lib, 4, layout)
        assert rc == EINVAL and h == 0
    with torch.cuda.device(cuda):
        rc, h, _ = _create(lib, 2, 1)
    assert rc == 0 and _probe(lib, h)[0] == 2
    assert lib.pwclo_stream_set_destroy(h) == 0
    k, lay, mask, ns = ctypes.c_int(5), ctypes.c_int(5), ctypes.c_uint(5), ctypes.c_longlong(5)
    assert lib.pwclo_stream_set_concurrency(h, ctypes.byref(k)) == EINVAL and k.value == 0
    assert lib.pwclo_stream_set_probe(h, ctypes.byref(lay), ctypes.byref(mask), ctypes.byref(ns)) == EINVAL
    assert (lay.value, mask.value, ns.value) == (0, 0, 0)
    p = ctypes.c_void_p()
    assert lib.pwclo_stream_set_stream(h, 0, ctypes.byref(p)) == EINVAL      # ... as by the old entry points
    assert lib.pwclo_stream_set_destroy(h) == EINVAL


@pytest.mark.parametrize("value", T.VALUES)
def test_pipelined_poses_are_the_serial_ones_under_every_priority_value(cuda, value):
    """One fresh child per value (started, not exec'd), one after another: 9 calls at depth 4, batch 2, 2 x 1024 points."""
    env = dict(os.environ, PWCLO_PIPE_PRIORITY=value)
    env.pop("PWCLO_PIPE_STREAMS", None)
    try:
        out = subprocess.run([sys.executable, os.path.join(T.ROOT, "tests", "pipe_priority_cases.py")], env=env, cwd=T.ROOT,
                             capture_output=True, text=True, timeout=180)
    except subprocess.TimeoutExpired:
        pytest.exit("the PWCLO_PIPE_PRIORITY=%s child hung: nothing more is started on this GPU" % value, returncode=3)
    print(out.stdout)
    if out.returncode < 0 or out.returncode in (134, 137, 139):      # killed by a signal: a fault, not a difference
        pytest.exit("the PWCLO_PIPE_PRIORITY=%s child died (%d): nothing more is started on this GPU\n%s"
                    % (value, out.returncode, out.stderr[-2000:]), returncode=3)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
    assert len(lines) == 1
    r = json.loads(lines[0][len("RESULT "):])
    assert r["asked"] == value and r["differ"] == [] and r["ok"] and T.consistent(r)
    assert 1 <= r["lanes"] <= 4


@pytest.fixture(scope="module")
def served(cuda):
    """The net, five inputs and their serial ``GraphedForward`` poses, shared by the two in-process pipeline tests."""
    net = T.make_net(cuda)
    inputs = T.make_inputs(cuda)[:5]
    return net, inputs, T.serial_poses(net, inputs)


def test_a_process_that_chose_no_layout_keeps_normal_streams_and_the_formula(cuda, served, monkeypatch):
    """No ``PWCLO_PIPE_PRIORITY`` and no ``configure_hw_queues()``: the set is a normal one, it still measures, and the
    pipeline rotates over the first ``lanes(depth)`` streams as it did before the layouts existed."""
    monkeypatch.setattr(pipe_streams, "_priority", pipe_streams.FORMULA)
    monkeypatch.setattr(pipe_streams, "_mode", "native")
    net, inputs, refs = served
    pipe, got = T.pipelined_poses(net, inputs)
    d = pipe.describe()
    print(d)
    assert d["streams"] == "native" and d["layout"] == "normal" and d["follows_probe"] is False
    assert 1 <= d["side_by_side"] <= 4 and len(d["together"]) == d["side_by_side"]
    assert d["lanes"] == d["formula_lanes"] == pipe_streams.lanes(4) and d["stream_indices"] == tuple(range(d["lanes"]))
    for c in range(len(inputs)):
        assert torch.equal(got[c], refs[c]), "call %d differs from GraphedForward" % c


def test_auto_reports_a_layout_whose_probe_value_is_the_lane_count_it_uses(cuda, served, monkeypatch):
    """In this process (whatever streams the tests before it made): ``auto`` on the set behind a depth-4 pipeline."""
    monkeypatch.setattr(pipe_streams, "_priority", "auto")
    monkeypatch.setattr(pipe_streams, "_mode", "native")
    net, inputs, refs = served
    pipe, got = T.pipelined_poses(net, inputs)
    d = pipe.describe()
    print(d)
    assert T.consistent(d) and d["follows_probe"] is True
    assert d["layout"] == pipe._set.layout and d["side_by_side"] == pipe._set.side_by_side == d["lanes"]
    assert d["layout"] == "normal" or d["side_by_side"] == 4
    used = {pipe._where[s]._pwclo_index for s in range(4) if pipe._where[s] is not None}
    assert used <= set(d["stream_indices"])
    for c in range(len(inputs)):
        assert torch.equal(got[c], refs[c]), "call %d differs from GraphedForward" % c
