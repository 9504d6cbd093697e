"""Every kernel instantiation of csrc/knn.hip against the oracle, bit for bit (run with ``-m gpu``).

Each case of tests/knn_cases.py first asserts through knn_point_plan_query -- the launchers' own selection code -- that its
shape launches the instantiations it is meant for, then runs its entry point and requires indices AND keys to be
``torch.equal`` to ``oracle.ops.knn_point_with_dist``: same neighbours, same keys, lower index first on ties.  There is no
tolerance.  Cases on a search structure (rows and pruned kernels) are also compared with the same call on the exhaustive
kernel, so that a difference names the kernel it comes from.  The table covers the three exhaustive forms, the five build
forms with both sides of their n thresholds, the ten rows forms with both sides of every register-count boundary (in blocks,
up to the 272 blocks of n = 16384), the pruned kernel at K > 32 and -- in a child process started with PWCLO_KNN_ROWS=0 -- at
K <= 32, the prebuilt entry points at 64 <= n < 256, and clouds / queries chosen against the pruning margins: zero extent in
x or z, identical points, a line, one far outlier, world-scale offsets, clusters tighter than the 1e-8 under the square
root, queries on the box, far outside it and on the cluster centres.  The last test requires the table to reach every
instantiation the launchers can select.
"""
import os
import subprocess
import sys

import pytest
import torch

import knn_cases as T

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_knn_every_instantiation_equals_the_oracle(cuda, case):
    plan = T.plan_of(case, use_rows=True)
    assert T.instantiations(plan) == case.want, (case.name, T.resolve_n(case), plan)
    assert T.instantiations(T.plan_of(case)) == case.want, "PWCLO_KNN_ROWS is set in this process: the rows kernels are off"
    if isinstance(case.n, T.NBlk):
        assert plan["nblk"] == case.n.blocks
    xyz, new_xyz = T.make_inputs(case, extra_clouds=2 if case.entry == "slice" else 0)
    want = T.oracle(case, xyz, new_xyz)
    got = T.run(case, xyz, new_xyz, cuda)
    di, dd = T.differences(got, want)
    on_structure = plan["kernel"] != "exhaustive"
    ei = ed = 0
    if on_structure:
        ex = T.run(case, xyz, new_xyz, cuda, exhaustive=True)
        ei, ed = T.differences(ex, want)
    print("\n%s n=%d %s: %d indices, %d keys differ from the oracle%s"
          % (case.name, T.resolve_n(case), " + ".join(case.want), di, dd,
             "; exhaustive kernel: %d, %d" % (ei, ed) if on_structure else ""))
    assert (ei, ed) == (0, 0), "the exhaustive kernel differs from the oracle"
    assert (di, dd) == (0, 0), "%s differs from the oracle (the exhaustive kernel does not)" % case.want[-1]
    assert torch.equal(got[1].cpu(), want[1]) and torch.equal(got[0].cpu(), want[0])
    if on_structure:
        assert torch.equal(got[1], ex[1]) and torch.equal(got[0], ex[0])


@pytest.mark.parametrize("case", T.REFINER_CASES, ids=T.case_id)
def test_refiner_search_forms_equal_the_registration_model(cuda, case):
    """The two searches of the knn refiner at its smallest clouds, bit for bit against tests/icp_model.py's knn (fp32 keys in
    the header's order, equal keys by ascending index) and against the oracle."""
    import numpy as np

    import icp_model
    assert T.instantiations(T.plan_of(case, use_rows=True)) == case.want
    xyz, queries = T.refiner_inputs(case)
    dist, idx = T.run(case, xyz, queries, cuda)
    want = T.oracle(case, xyz, queries)
    assert torch.equal(idx.cpu(), want[1]) and torch.equal(dist.cpu(), want[0])
    for c in range(case.b):
        wi, wd = icp_model.knn(queries[c].numpy(), xyz[c].numpy(), case.k)
        assert np.array_equal(idx[c].cpu().numpy(), wi), c
        assert np.array_equal(dist[c].cpu().numpy().view(np.int32), wd.view(np.int32)), c


def test_pruned_kernel_serves_k_up_to_32_with_rows_off(cuda):
    """PWCLO_KNN_ROWS is read once per process, so K <= 32 on knn_pruned_kernel needs a process of its own: the child asserts
    through the plan query that its cases select the pruned kernel, compares K = 1, 6, 16, 32 on two cloud kinds with the
    oracle and exits non-zero on any difference.  (A few seconds: the import, eight small searches and their oracle.)"""
    env = dict(os.environ, PWCLO_KNN_ROWS="0")
    try:
        out = subprocess.run([sys.executable, os.path.join(T.ROOT, "tests", "knn_cases.py"), "--rows0"], env=env, cwd=T.ROOT,
                             capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        pytest.exit("the PWCLO_KNN_ROWS=0 child hung: nothing more is started on this GPU", returncode=3)
    print(out.stdout)
    if out.returncode < 0 or out.returncode in (134, 137, 139):      # killed by a signal: a fault, not a difference
        pytest.exit("the PWCLO_KNN_ROWS=0 child died (%d): nothing more is started on this GPU\n%s"
                    % (out.returncode, out.stderr[-2000:]), returncode=3)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    assert out.stdout.count("pruned differs from the oracle at 0 indices, 0 keys; exhaustive at 0, 0") == len(T.ROWS0_CASES)


def test_case_table_reaches_every_instantiation():
    """The instantiations the plan query names over the table (and the child's cases) are exactly those it can name for any
    shape the entry points accept (``knn_cases.selectable``: a sweep of the launchers' own selection) -- all 19.  A kernel
    added to the dispatch later without a case fails here."""
    reached = set()
    for case in T.CASES:
        reached.update(T.instantiations(T.plan_of(case, use_rows=True)))
    for case in T.ROWS0_CASES:
        reached.update(T.instantiations(T.plan_of(case, use_rows=False)))
    can = T.selectable()
    assert reached == can, ("not reached", sorted(can - reached), "not selectable", sorted(reached - can))
    assert reached == set(T.ALL_INSTANTIATIONS) and len(reached) == 19
