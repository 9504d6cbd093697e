"""The case tables of tests/test_gpu_eval_edges.py with their inputs, shared with tests/test_eval_cases_cpu.py, which proves that
they reach every class of the evaluation kernels' arithmetic and tell the host model (tests/eval_model.py) from each of its
planted faults.  CPU NumPy only; every input is a pure function of the table.

rows_to_transforms: n in ROWS_N pose rows whose quaternions go round QUAT_KINDS -- unit, norm 0.1, norm 10, zero, and three
built from fp32 components so that the kernel's float64 ``((w w + x x) + y y) + z z`` IS the float64 1e-8 of the identity
rule, the float64 below it, the float64 above it (``quat_with_norm2``; asserted where it is built).

accumulate / trajectory_distances: one launch over SCAN_LENGTHS = [0, 1, 2, 0, 63, 64, 65, 127, 128, 129, 0] (chunk 1, 2, 3;
lanes with empty chunks; empty sequences first, in the middle, last); about 1 m and a few degrees per frame; the sequence of
127 frames stands still over frames 40..59 (identity rows; ``scan_poses`` for the distances: tied bit for bit).

sequence_errors: ERROR_LENGTHS = [0, 7, 0, 90, 41, 0], SEGMENTS = (3, 5, 1000), STEPS = (1, 4, 10).  "metre": the ground truth
moves exactly 1 m per frame along x with the identity rotation and stands still over frames 20..29 of the long sequence, so
distances are exact integers, a 3 m segment ends exactly ON a travelled distance (the search is strict) and ties occur;
results: "same" (res = gt) and "drift" (res moves 1.0625 m per frame: t_err = 0.0625 (last - first) exactly).  "turning":
poses with rotation, results "same" (the trace of the error rounds above 1 in places: only the clamp keeps acos from NaN) and
"other" (another trajectory: r_err of a few degrees, the values the acos ulp figure is measured on).
"""
import numpy as np

import eval_model as EM

F32 = np.float32
ROWS_N = (1, 255, 257)
QUAT_KINDS = ("unit", "norm0.1", "norm10", "zero", "at_1e-8", "below_1e-8", "above_1e-8")
SCAN_LENGTHS = [0, 1, 2, 0, 63, 64, 65, 127, 128, 129, 0]
STILL_SEQ, STILL = 7, (40, 60)                 # SCAN_LENGTHS[7] = 127 frames, identity rows over [40, 60)
ERROR_LENGTHS = [0, 7, 0, 90, 41, 0]
SEGMENTS = (3.0, 5.0, 1000.0)
STEPS = (1, 4, 10)
METRE_STILL_SEQ, METRE_STILL = 3, (20, 30)
DRIFT = 1.0625
ERROR_CASES = [(world, result, step) for world, result in (("metre", "same"), ("metre", "drift"), ("turning", "same"),
                                                           ("turning", "other")) for step in STEPS]


def quat_with_norm2(target):
    """fp32 (w, x, y, 0) whose ((w w + x x) + y y) + 0 in float64 is exactly ``target`` (about 1e-8): w just below the
    root, x closes most of the gap, y the rest (y y is far finer than an ulp of the target)."""
    target = np.float64(target)
    w = np.nextafter(F32(np.sqrt(target)), F32(0))
    wd = np.float64(w)
    x = F32(np.sqrt(target - wd * wd))
    while wd * wd + np.float64(x) * np.float64(x) >= target:
        x = np.nextafter(x, F32(0))
    a = wd * wd + np.float64(x) * np.float64(x)
    y0 = F32(np.sqrt(target - a))
    for k in range(-64, 65):
        y = y0
        for _ in range(abs(k)):
            y = np.nextafter(y, F32(np.inf if k > 0 else 0))
        q = np.array([w, x, y, 0], dtype=F32)
        if ((np.float64(q[0]) ** 2 + np.float64(q[1]) ** 2) + np.float64(q[2]) ** 2) + 0.0 == target:
            return q
    raise AssertionError("no fp32 quaternion with squared norm %r" % target)


def _unit(rng, n, max_deg):
    """(n, 4) float64 unit quaternions of rotations by up to max_deg about random axes."""
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    half = np.deg2rad(rng.uniform(-max_deg, max_deg, size=n)) / 2
    return np.concatenate((np.cos(half)[:, None], np.sin(half)[:, None] * axis), axis=1)


def pose_rows(n, seed, max_deg=4.0):
    """(n, 7) fp32 [t, q]: about 1 m forward and up to max_deg per frame."""
    rng = np.random.default_rng(seed)
    t = np.stack((rng.uniform(0.8, 1.2, n), rng.uniform(-0.05, 0.05, n), rng.uniform(-0.1, 0.1, n)), axis=1)
    return np.concatenate((t, _unit(rng, n, max_deg)), axis=1).astype(F32)


def quat_rows(n):
    """(n, 7) fp32 rows with the quaternions of QUAT_KINDS in turn, and the kind of every row."""
    rows = pose_rows(n, 300 + n, 170.0)
    edge = {"at_1e-8": quat_with_norm2(1e-8), "below_1e-8": quat_with_norm2(np.nextafter(1e-8, 0.0)),
            "above_1e-8": quat_with_norm2(np.nextafter(1e-8, 1.0))}
    kinds = [QUAT_KINDS[i % len(QUAT_KINDS)] for i in range(n)]
    for i, kind in enumerate(kinds):
        if kind == "norm0.1":
            rows[i, 3:] *= F32(0.1)
        elif kind == "norm10":
            rows[i, 3:] *= F32(10.0)
        elif kind == "zero":
            rows[i, 3:] = 0
        elif kind in edge:
            rows[i, 3:] = edge[kind]
    return rows, kinds


IDENTITY_ROW = np.array([0, 0, 0, 1, 0, 0, 0], dtype=F32)


SCAN_SEED = 41
YARDSTICK_SEEDS = (SCAN_SEED, 1, 2, 3, 4, 5, 6, 7, 8)      # tests/test_eval_cases_cpu.py: the plain loop's typical error


def scan_rows(seed=SCAN_SEED):
    """(sum(SCAN_LENGTHS), 7) fp32 pose rows of all sequences back to back."""
    rows = pose_rows(sum(SCAN_LENGTHS), seed)
    lo = int(np.sum(SCAN_LENGTHS[:STILL_SEQ]))
    rows[lo + STILL[0]:lo + STILL[1]] = IDENTITY_ROW
    return rows


def scan_transforms(seed=SCAN_SEED):
    return EM.rows_to_transforms(scan_rows(seed))


def scan_poses():
    """The poses the distance kernel is given: the model's trajectories of ``scan_transforms`` with the stationary stretch
    made exactly stationary (the scan re-associates the products, so multiplying by the identity still moves a pose by a
    rounding; copies of one pose give distances that tie bit for bit)."""
    poses = EM.accumulate(scan_transforms(), SCAN_LENGTHS)
    lo = int(np.sum(SCAN_LENGTHS[:STILL_SEQ]))
    poses[lo + STILL[0]:lo + STILL[1]] = poses[lo + STILL[0] - 1]
    return poses


def _metre(result):
    """ERROR_LENGTHS sequences of (n, 4, 4) poses: x = frames moved so far (the still stretch does not move) times the
    result's metres per frame."""
    out = []
    for s, n in enumerate(ERROR_LENGTHS):
        moved = np.ones(n)
        if n:
            moved[0] = 0.0
        if s == METRE_STILL_SEQ:
            moved[METRE_STILL[0]:METRE_STILL[1]] = 0.0
        pose = np.tile(np.eye(4), (n, 1, 1))
        pose[:, 0, 3] = np.cumsum(moved) * (DRIFT if result == "drift" else 1.0) + (2.0 if n else 0.0)
        out.append(pose)
    return np.concatenate(out)


def _turning(seed):
    rows = pose_rows(sum(ERROR_LENGTHS), seed, 6.0)
    return EM.accumulate(EM.rows_to_transforms(rows), ERROR_LENGTHS)


def error_inputs(world, result):
    """-> (gt (N, 4, 4), res (N, 4, 4), dist (N,)): dist is the model's scan of the ground truth."""
    if world == "metre":
        gt, res = _metre("same"), _metre(result)
    else:
        gt = _turning(77)
        res = gt.copy() if result == "same" else _turning(78)
    return gt, res, EM.distances(gt, ERROR_LENGTHS)
