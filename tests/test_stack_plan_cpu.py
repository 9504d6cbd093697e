"""The case table of tests/test_gpu_stack_variants.py, checked on a machine without a GPU: every row of
``stack_cases.CASES`` / ``CHILD_CASES`` runs as a DRY run on CPU tensors -- the wrappers' whole dispatch, argument guards
included, with the launch itself left out (include/pwclo_ops.h: pwclo_set_dry_run) -- and must record exactly the kernel
instantiations it names.  The names come from the runtime's symbol of the kernel the launch layer was instantiated with,
demangled: the table's strings are compared with them in all three weight formats, with ``bool`` and with defaulted
template arguments.  Further: the record's contract (taken once, none for a call that launched nothing or failed) and
the grid rule of csrc/launch.hpp, launch_persistent.  Needs the built library, like the other *_plan_cpu tests.
"""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":                       # the child process: no conftest to set the paths up
    sys.path[:0] = [os.path.dirname(HERE), HERE]

from pwclonet_pylidarslam_amd import _lib, fused                                 # noqa: E402
from stack_cases import CASES, CHILD_CASES, CHILD_ENV, launched                  # noqa: E402

CPU = torch.device("cpu")


def dry_names(case):
    with fused.packing_dtype(case.fmt):
        return [r[1] for r in launched(case, CPU, dry=True)[1]]


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_row_launches_the_kernels_it_names(monkeypatch, case):
    for k, v in case.setenv.items():
        monkeypatch.setenv(k, v)
    assert dry_names(case) == case.want


def test_switched_off_rows_in_a_child_process():
    """CHILD_ENV's switches are read once per process: one fresh CPU child prints what each CHILD_CASES row recorded."""
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, **CHILD_ENV),
                           capture_output=True, text=True, timeout=120)
    assert child.returncode == 0, "child exited with %d:\n%s" % (child.returncode, child.stderr[-4000:])
    rows = [json.loads(line) for line in child.stdout.splitlines() if line.startswith("[")]
    assert rows == [c.want for c in CHILD_CASES]


def test_table_names_every_format_bool_and_defaulted_arguments():
    wants = {w for c in CASES + CHILD_CASES for w in c.want}
    for name in ("cv_a2_kernel<8, 1, 16, 0>",                       # FMT defaulted in the wrapper's text
                 "cv_a2_kernel<32, 2, 8, 1>", "cv_a2_kernel<32, 2, 8, 2>",
                 "sa_h_kernel<1, 1, 2, 32, 2, 8, false, 0, false>",  # KMAJ defaulted
                 "sa_h_kernel<1, 1, 1, 32, 2, 8, true, 0, true>", "cv_a_lane6_kernel<8, false>",
                 "pointwise_kernel<4, 4, 4, 8, 4, 2, 8, 0>",        # BT defaulted
                 "linear_jobs_kernel"):                             # no template
        assert name in wants, name


# ---- the record's contract ---------------------------------------------------------------------------------------

def pointwise_args(b, s, c0=64, c1=64, c2=0, w1=64, w2=0):
    return (b, s, c0, c1, c2, w1, w2, 0, 0, 0, 0, 0)


def take(lib):
    buf, geo = ctypes.create_string_buffer(256), (ctypes.c_int * 4)()
    return (buf.value.decode(), list(geo)) if lib.pwclo_take_launch(buf, len(buf), geo) else None


@pytest.fixture
def dry_lib():
    lib = _lib.load()
    lib.pwclo_take_launch(None, 0, None)
    lib.pwclo_set_dry_run(1)
    yield lib
    lib.pwclo_set_dry_run(0)
    lib.pwclo_clear_error()


def test_record_is_handed_out_once(dry_lib):
    assert take(dry_lib) is None
    dry_lib.pointwise_fused_kernel_wrapper(*pointwise_args(2, 203))
    assert dry_lib.pwclo_last_error() == 0
    # Stack<8, 4>: 4 x (4 * 8 * 256 + 4 * 16) bytes; 26 tiles on 4-wave workgroups
    assert take(dry_lib) == ("pointwise_kernel<4, 4, 0, 4, 0, 1, 4, 0>", [4, 7, 1, 33024])
    assert take(dry_lib) is None
    dry_lib.pointwise_fused_kernel_wrapper(*pointwise_args(2, 203))
    assert dry_lib.pwclo_take_launch(None, 0, None) == 1 and take(dry_lib) is None      # both outputs are optional
    small = ctypes.create_string_buffer(10)
    dry_lib.pointwise_fused_kernel_wrapper(*pointwise_args(2, 203))
    assert dry_lib.pwclo_take_launch(small, len(small), None) == 1 and small.value == b"pointwise"     # truncated, terminated


def test_call_that_launches_nothing_leaves_no_record(dry_lib):
    dry_lib.pointwise_fused_kernel_wrapper(*pointwise_args(0, 203))
    assert dry_lib.pwclo_last_error() == 0 and take(dry_lib) is None
    with _lib.launches(dry=True) as rec:
        _lib.call("pointwise_fused_kernel_wrapper", CPU, *pointwise_args(0, 203))
        _lib.call("linear_jobs_kernel_wrapper", CPU, 0, None, None, None, None, None, None, None)
    assert rec == []


def test_failed_call_leaves_no_record_and_raises_as_before(dry_lib):
    dry_lib.pointwise_fused_kernel_wrapper(*pointwise_args(2, 203))        # an earlier call's record, not taken
    dry_lib.pointwise_fused_kernel_wrapper(*pointwise_args(2, 203, c1=48))
    assert dry_lib.pwclo_last_error() == 10001 and take(dry_lib) is None
    dry_lib.pwclo_clear_error()
    with _lib.launches(dry=True) as rec:
        _lib.call("pointwise_fused_kernel_wrapper", CPU, *pointwise_args(2, 203))
        with pytest.raises(RuntimeError, match=r"pointwise_fused: no kernel for sources \(64,48,0\)"):
            _lib.call("pointwise_fused_kernel_wrapper", CPU, *pointwise_args(2, 203, c1=48))
    assert [r[:2] for r in rec] == [("pointwise_fused_kernel_wrapper", "pointwise_kernel<4, 4, 0, 4, 0, 1, 4, 0>")]
    assert dry_lib.pwclo_last_error() == 0 and take(dry_lib) is None


def test_launches_restores_the_flag_and_nests():
    lib = _lib.load()
    with _lib.launches(dry=True) as outer:
        with _lib.launches(dry=True) as inner:
            _lib.call("pointwise_fused_kernel_wrapper", CPU, *pointwise_args(2, 203))
        _lib.call("pointwise_fused_kernel_wrapper", CPU, *pointwise_args(2, 16391))
    assert [r[1] for r in inner] == ["pointwise_kernel<4, 4, 0, 4, 0, 1, 4, 0>"]
    assert [r[1] for r in outer] == ["pointwise_kernel<4, 4, 0, 4, 0, 1, 16, 0>"]
    assert _lib._recording is None and _lib._dry is False and take(lib) is None


# ---- the grid rule -----------------------------------------------------------------------------------------------

def layer_floats(nbi, nbo):
    return nbo * nbi * 256 + nbo * 16


def test_persistent_grid_rule():
    """csrc/launch.hpp, launch_persistent: one workgroup per W tiles, at most 256 x per_cu x rounds (rounds = 1 for these
    wrappers), per_cu = 1 when the stack needs more than 80 KiB of LDS or the workgroup has more than 8 waves, else 2."""
    small, big = 4 * (layer_floats(8, 4)), 4 * (layer_floats(12, 8) + layer_floats(8, 4))
    assert small <= 80 * 1024 < big
    psa2 = layer_floats(1, 1) + layer_floats(1, 1) + layer_floats(1, 2)
    dummy = torch.zeros(4)
    rows = [
        # 16384 tiles on 16 waves: 1024 workgroups wanted, a wide workgroup has its CU to itself -> 256
        ("pointwise_fused_kernel_wrapper", pointwise_args(32, 8192), ("pointwise_kernel<4, 4, 0, 4, 0, 1, 16, 0>", 16, (256, 1), small)),
        # 2050 tiles on 16 waves: 129 workgroups, below the cap
        ("pointwise_fused_kernel_wrapper", pointwise_args(2, 16391), ("pointwise_kernel<4, 4, 0, 4, 0, 1, 16, 0>", 16, (129, 1), small)),
        # 2047 tiles on 4 waves, small stack: 512 workgroups = 256 x 2
        ("pointwise_fused_kernel_wrapper", pointwise_args(1, 16 * 2047), ("pointwise_kernel<4, 4, 0, 4, 0, 1, 4, 0>", 4, (512, 1), small)),
        # the same tiles with a 129 KiB stack: one workgroup per CU -> 256
        ("pointwise_fused_kernel_wrapper", pointwise_args(1, 16 * 2047, 128, 64, 0, 128, 64),
         ("pointwise_kernel<8, 4, 0, 8, 4, 1, 4, 0>", 4, (256, 1), big)),
        # psa_2, 3 x 5000 tiles of 2 x 16 pixels on 8 waves: 1875 workgroups wanted, tiny stack -> 512
        ("sa_fused_h_kernel_wrapper", (3, 9000, 5000, 20, 16, 16, 32, 0, 0, dummy.data_ptr(), 0, 0, 0, 0, psa2, 0),
         ("sa_h_kernel<1, 1, 2, 32, 2, 8, false, 0, false>", 8, (512, 1), 4 * psa2)),
        # no tiles to speak of: never less than one workgroup
        ("pointwise_fused_kernel_wrapper", pointwise_args(1, 1), ("pointwise_kernel<4, 4, 0, 4, 0, 1, 4, 0>", 4, (1, 1), small)),
    ]
    with _lib.launches(dry=True) as rec:
        for name, args, _ in rows:
            _lib.call(name, CPU, *args)
    assert rec == [(name,) + want for name, _, want in rows]
    # linear jobs: its own 2-D grid (blockIdx.y = job), ceil(ceil(500 / 32) / 8) = 2 workgroups of 8 waves per job
    with _lib.launches(dry=True) as rec:
        fused.run_linear_jobs([(fused.LinearJob(torch.zeros(128, 16), torch.zeros(128)), torch.zeros(1, 500, 16)),
                               (fused.LinearJob(torch.zeros(64, 32), torch.zeros(64)), torch.zeros(1, 33, 32))])
    assert rec == [("linear_jobs_kernel_wrapper", "linear_jobs_kernel", 8, (2, 2), 4 * layer_floats(1, 8))]


if __name__ == "__main__":
    assert sys.argv[1:] == ["--child"]
    for case_ in CHILD_CASES:
        print(json.dumps(dry_names(case_)), flush=True)
