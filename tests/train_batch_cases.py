"""Case tables for the training batch builder's kernels (csrc/train_batch.hip): a test helper, not a
conftest and not a product module.  No GPU, no randomness at import: every case is a small dict, ``materialise`` turns it
into the arrays ``TrainBatchBuilder.build`` and ``train_batch_model.build`` take.  tests/test_train_batch_cases_cpu.py proves
that each table reaches what it names and tells every planted fault of the model from the model;
tests/test_gpu_train_batch_edges.py runs the same tables through the kernels.

Rows survive or not by construction: a survivor has |x| < 16, |y| < 13, |z| <= 0.5 (inside both datasets' boxes, through
``VELO_TO_CAM`` for KITTI: (-y, -z, x)), a non-survivor has x = 100.  All coordinates are multiples of 1/128, exact in fp32
and under the permutation calibration, and differ from row to row, so a wrong row shows in the coordinates as well.

Tables
* PADDING        npoints that are no power of two (P > npoints: all-ones padding, sort over P slots), and 1, 2.
* COUNTS         count in {0, 1, npoints - 1, npoints, npoints + 1} at npoints = 100 (P = 128) and 128 (P = npoints).
* ROW_EDGES      n in {1, 63, 64, 65, 1023, 1024, 1025, 1089} and n = 4096 with the survivors in one wave's range.
* DEVICE_LENGTHS lengths as a device tensor: 0, negative, beyond R, and a short frame, next to an ordinary pair.
* TIES           two survivors with the same 32-bit Philox word at, below and above the selection threshold.
* QUAT, EULER    every branch of both quaternion forms, exact ties of the branch choice, the gimbal threshold.
* WIDE           B = 257 pairs: the pose kernel's second trip through its ``b += 256`` loop.

Ties.  Philox words cannot be planted, so equal words were searched for once (``find_collisions``: all 2^18 words of a
(seed, step, cloud), sorted) and the finds are committed in ``COLLISIONS``; the CPU test recomputes them.  "cross": the two
rows lie in different waves' ranges; "same": in one wave's range, in different 64-row steps; "dense": all 2^18 rows survive
and the colliding word has rank < 8192 among them, the real regime (full histograms, a threshold deep in the last digit).
A pair inside one 64-row step would need a collision within 64 rows; none was searched for.  That sub-path differs from the
"same" case only in that both rows meet in one ballot, where ``mbcnt64`` ranks them instead of the running ``tie_base`` the
"same" case already carries from one step to the next.
"""
import numpy as np

import train_batch_model as model

VELO_TO_CAM = np.array([[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0], [1.0, 0.0, 0.0, 0.0]])
DATASETS = ("kitti", "kitti360")
SEED = 11
TIE_R = 1 << 18
EPS4 = 4.0 * np.finfo(np.float64).eps

COLLISIONS = {
    "cross": dict(seed=11, step=0, cloud=0, rows=(61733, 238311), word=0x2CC031D6),
    "same": dict(seed=11, step=1, cloud=0, rows=(182698, 184704), word=0x7EEA6D99),
    "dense": dict(seed=11, step=2, cloud=1, rows=(113371, 142604), word=0x049A38E9, rank=4659),
}


def find_collisions(seed, step, cloud, rows=TIE_R):
    """Every pair of rows of one cloud whose selection words are equal: [dict(rows=(i, j), word, rank)], i < j, rank = the
    number of smaller words among all ``rows``.  How ``COLLISIONS`` was found (seed 11, steps 0-5, clouds 0 and 1); not run
    at import."""
    w = model.words(np.arange(rows), cloud, step, model.SELECT, seed)
    order = np.argsort(w, kind="stable")
    ws = w[order]
    found = []
    for e in np.nonzero(ws[1:] == ws[:-1])[0]:
        found.append(dict(rows=(int(order[e]), int(order[e + 1])), word=int(ws[e]), rank=int((w < ws[e]).sum())))
    return found


# ---- rows -------------------------------------------------------------------------------------------------------------------
def raw_rows(R, cloud):
    """(R, 4) float32 rows that all survive both filters; distinct (x, y) for R < 2039 * 1543."""
    i = np.arange(R, dtype=np.int64)
    out = np.empty((R, 4), dtype=np.float32)
    out[:, 0] = ((i * 37 + cloud * 11) % 2039) / 64.0 - 15.9375
    out[:, 1] = ((i * 53 + cloud * 7) % 1543) / 64.0 - 12.0
    out[:, 2] = ((i * 29 + cloud) % 127) / 128.0 - 0.5
    out[:, 3] = (i % 256) / 256.0
    return out


def tie_survivors(key, smaller=5, larger=5):
    """The colliding pair of ``COLLISIONS[key]`` plus ``smaller`` rows with smaller and ``larger`` rows with larger words,
    spread over the frame (first, quartiles, last of each kind, so one smaller-word row lies behind the pair)."""
    c = COLLISIONS[key]
    w = model.words(np.arange(TIE_R), c["cloud"], c["step"], model.SELECT, c["seed"])
    rows = list(c["rows"])
    for idx, k in ((np.nonzero(w < c["word"])[0], smaller), (np.nonzero(w > c["word"])[0], larger)):
        rows += [int(idx[(len(idx) - 1) * q // (k - 1)]) for q in range(k)]
    return sorted(rows)


def keep_mask(spec, R):
    """A survivor spec -> (R,) bool.  ("all",), ("none",), ("spread", count, n): count rows evenly over [0, n),
    ("except", k, r): rows with i % k != r, ("range", lo, hi, k, r): those of them in [lo, hi), ("tie", key)."""
    i = np.arange(R)
    kind = spec[0]
    if kind == "all":
        return np.ones(R, dtype=bool)
    if kind == "none":
        return np.zeros(R, dtype=bool)
    if kind == "spread":
        keep = np.zeros(R, dtype=bool)
        keep[(np.arange(spec[1]) * spec[2]) // max(spec[1], 1)] = True
        return keep
    if kind == "except":
        return i % spec[1] != spec[2]
    if kind == "range":
        return (i >= spec[1]) & (i < spec[2]) & (i % spec[3] != spec[4])
    if kind == "tie":
        keep = np.zeros(R, dtype=bool)
        keep[tie_survivors(spec[1])] = True
        return keep
    raise ValueError(spec)


def rot(axis, angle):
    """Rodrigues' formula in fp64."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.sqrt(a.dot(a))
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * K.dot(K)


def motions(B):
    """(B, 4, 4) f64: small, distinct relative motions for the selection tables."""
    T = np.tile(np.eye(4), (B, 1, 1))
    for b in range(B):
        T[b, :3, :3] = rot((0.1 * ((b % 7) - 3), 0.3, 1.0), 0.02 * ((b % 11) + 1))
        T[b, :3, 3] = (0.5 + 0.01 * b, 0.1 - 0.003 * b, -0.05)
    return T


def given_params(B):
    """(B, 6) f32 inside the clips, different for every pair and parameter."""
    k = np.arange(B * 6).reshape(B, 6)
    return (((k * 37) % 2003 - 1001) / 1001.0 * model.AUG_CLIP).astype(np.float32)


# ---- selection tables -------------------------------------------------------------------------------------------------------
def _sel(table, name, dataset, npoints, R, lengths, survivors, step=3, seed=SEED, device_lengths=False, **more):
    return dict(table=table, name="%s-%s-%s" % (table, name, dataset), dataset=dataset, npoints=npoints, R=R,
                lengths=[list(v) for v in lengths], survivors=survivors, step=step, seed=seed,
                device_lengths=device_lengths, mode=1, **more)


PADDING_NPOINTS = (1, 2, 3, 5, 1000, 1025, 4097)
COUNT_NPOINTS = (100, 128)
ROW_EDGE_N = (1, 63, 64, 65, 1023, 1024, 1025, 1089)
ROW_EDGE_WAVES = {1: 1, 63: 1, 64: 1, 65: 2, 1023: 16, 1024: 16, 1025: 9, 1089: 9}      # non-empty ranges: 0 .. k-1
DEVICE_R = 200


def padding_cases():
    out = []
    for ds in DATASETS:
        for m in PADDING_NPOINTS:
            n = 3 * m + 7
            sp = ("spread", 2 * m + 1, n)
            out.append(_sel("padding", "np%d" % m, ds, m, n, [(n, n)], [(sp, sp)]))
    return out


def count_cases():
    out = []
    for ds in DATASETS:
        for m in COUNT_NPOINTS:
            n, counts = 333, (0, 1, m - 1, m, m + 1)
            sv = [(("spread", c, n),) * 2 if c else (("none",),) * 2 for c in counts]
            out.append(_sel("counts", "np%d" % m, ds, m, n, [(n, n)] * 5, sv, counts=counts))
    return out


def row_edge_cases():
    """One batch per dataset, npoints = 16, R = 4096: pair k cut to ROW_EDGE_N[k] rows (the shorter frame alternates), then
    two pairs of 4096 rows whose survivors lie in wave 0's range [0, 256) and in wave 15's [3840, 4096)."""
    out = []
    for ds in DATASETS:
        R = 4096
        lengths = [(n, R) if k % 2 else (min(n + 3, R), n) for k, n in enumerate(ROW_EDGE_N)] + [(R, R), (R, R)]
        sv = [(("except", 5, 1),) * 2] * len(ROW_EDGE_N) + [(("range", 0, 256, 3, 0),) * 2, (("range", 3840, 4096, 3, 0),) * 2]
        out.append(_sel("row_edges", "np16", ds, 16, R, lengths, sv, n=list(ROW_EDGE_N) + [R, R]))
    return out


def device_length_cases():
    """(0, 5) and (-3, 7) clamp to n = 0; (R + 9, R + 1) to R, with no survivor in frame 1 so that its draws are over n
    itself; (7, R) is a short frame; (150, 180) an ordinary pair."""
    R = DEVICE_R
    ex = ("except", 5, 1)
    lengths = [(0, 5), (-3, 7), (R + 9, R + 1), (7, R), (150, 180)]
    sv = [(ex, ex), (ex, ex), (ex, ("none",)), (ex, ex), (ex, ex)]
    return [_sel("device_lengths", "np16", ds, 16, R, lengths, sv, device_lengths=True, n=[0, 0, R, 7, 150]) for ds in DATASETS]


def tie_cases():
    """npoints counts from the 5 smaller-word survivors of ``tie_survivors``: 6 = the pair is at the threshold and one of the
    two is needed; 7 = both; 9 = the threshold is the second larger word; 3 = the third smaller one."""
    out = []

    def sparse(name, key, ds, m, ties, need, take, leave):
        c = COLLISIONS[key]
        sv = ("tie", key)
        return _sel("ties", name, ds, m, TIE_R, [(TIE_R, TIE_R)], [(sv, sv)], step=c["step"], seed=c["seed"], key=key,
                    ties=ties, need=need, take=take, leave=leave)

    (i, j), (k, l) = COLLISIONS["cross"]["rows"], COLLISIONS["same"]["rows"]
    out.append(sparse("cross_one_of_two", "cross", "kitti360", 6, 2, 1, (i,), (j,)))
    out.append(sparse("cross_one_of_two", "cross", "kitti", 6, 2, 1, (i,), (j,)))
    out.append(sparse("same_one_of_two", "same", "kitti360", 6, 2, 1, (k,), (l,)))
    out.append(sparse("cross_both", "cross", "kitti360", 7, 2, 2, (i, j), ()))
    out.append(sparse("cross_below", "cross", "kitti360", 9, 1, 1, (i, j), ()))
    out.append(sparse("cross_above", "cross", "kitti360", 3, 1, 1, (), (i, j)))
    c = COLLISIONS["dense"]
    for name, ds, m, need, take, leave in (("dense_one_of_two", "kitti360", c["rank"] + 1, 1, c["rows"][:1], c["rows"][1:]),
                                           ("dense_one_of_two", "kitti", c["rank"] + 1, 1, c["rows"][:1], c["rows"][1:]),
                                           ("dense_both", "kitti360", c["rank"] + 2, 2, c["rows"], ())):
        out.append(_sel("ties", name, ds, m, TIE_R, [(TIE_R, TIE_R)], [(("all",),) * 2], step=c["step"], seed=c["seed"],
                        key="dense", ties=2, need=need, take=tuple(take), leave=tuple(leave)))
    return out


def selection_cases():
    return padding_cases() + count_cases() + row_edge_cases() + device_length_cases() + tie_cases()


# ---- pose tables ------------------------------------------------------------------------------------------------------------
def _perm(*rows):
    return np.array(rows, dtype=np.float64)


def _skew170(i):
    axis = [0.3, 0.3, 0.3]
    axis[i] = 0.9
    return rot(axis, np.radians(170.0))


# name -> (rotation, branch: 0, 1, 2 = m00, m11, m22, 3 = trace; the FIRST largest where several are equal)
QUAT_ROTATIONS = [
    ("half_turn_x", np.diag([1.0, -1.0, -1.0]), 0),
    ("half_turn_y", np.diag([-1.0, 1.0, -1.0]), 1),
    ("half_turn_z", np.diag([-1.0, -1.0, 1.0]), 2),
    ("skew170_m00", _skew170(0), 0),
    ("skew170_m11", _skew170(1), 1),
    ("skew170_m22", _skew170(2), 2),
    ("small", rot((0.3, -0.5, 0.8), 0.05), 3),
    ("identity", np.eye(3), 3),
    ("third_turn", _perm((0, 0, 1), (1, 0, 0), (0, 1, 0)), 0),                # 120 degrees about (1,1,1): all four are 0
    ("third_turn_back", _perm((0, 1, 0), (0, 0, 1), (1, 0, 0)), 0),           # -120: the branches differ in sign here
    ("quarter_z", _perm((0, -1, 0), (1, 0, 0), (0, 0, 1)), 2),                # m22 == trace == 1
    ("quarter_z_back", _perm((0, 1, 0), (-1, 0, 0), (0, 0, 1)), 2),
    ("quarter_x_back", _perm((1, 0, 0), (0, 0, 1), (0, -1, 0)), 0),           # m00 == trace
    ("quarter_y_back", _perm((0, 0, -1), (0, 1, 0), (1, 0, 0)), 1),           # m11 == trace
]
QUAT_TIES = ("third_turn", "third_turn_back", "quarter_z", "quarter_z_back", "quarter_x_back", "quarter_y_back")


def _pitch(sy, cy, sz=0.0, cz=1.0, proper=True):
    """Ry(pitch) . Rz(yaw) from the sines and cosines themselves (so cos(pitch) is exactly what is asked for); with
    ``proper=False`` the entries cy * cz, cy * sz of row 0 are left 0, which makes the two Euler branches tell apart."""
    a, b = (cy * cz, -cy * sz) if proper else (0.0, 0.0)
    return np.array([[a, b, sy], [sz, cz, 0.0], [-sy * cz, sy * sz, cy]], dtype=np.float64) + 0.0      # no -0.0 entries


ABOVE = float(np.nextafter(EPS4, 1.0))
# name -> (rotation, gimbal branch taken)
EULER_ROTATIONS = [
    ("pitch_up", _pitch(1.0, 0.0), True),                                     # [[0,0,1],[0,1,0],[-1,0,0]]: c == 0
    ("pitch_down", _pitch(-1.0, 0.0), True),
    ("pitch_up_yaw", _pitch(1.0, 0.0, 0.6, 0.8), True),                       # c == 0 with a yaw only the gimbal branch sees
    ("pitch_down_yaw", _pitch(-1.0, 0.0, 0.6, 0.8), True),
    ("delta_above", _pitch(1.0, 1e-15, 0.6, 0.8), False),                     # pitch 90 degrees - 1e-15 rad: c > 4 eps
    ("delta_below", _pitch(1.0, 8e-16, 0.6, 0.8), True),                      # - 8e-16 rad: c < 4 eps
    ("edge_at", _pitch(1.0, EPS4, 0.6, 0.8, proper=False), True),             # c == 4 eps: not above it
    ("edge_above", _pitch(1.0, ABOVE, 0.6, 0.8, proper=False), False),        # one ulp more
    ("large_yaw_roll", rot((1, 0, 0), 2.5).dot(rot((0, 1, 0), -0.7)).dot(rot((0, 0, 1), -2.9)), False),
    ("large_yaw", rot((0, 0, 1), 2.2).dot(rot((1, 0, 0), -1.9)), False),
]
POSE_TRANSLATION = (1.5, -0.25, 0.75)


def pose_cases():
    """Both rotation lists under both datasets (the other dataset's form runs on the same matrices), mode 0 (T_gt = T_diff
    bit for bit) and mode 2 (composed with ``given_params``)."""
    out = []
    ex = ("except", 5, 1)
    for table, rots in (("quat", QUAT_ROTATIONS), ("euler", EULER_ROTATIONS)):
        for ds in DATASETS:
            for mode in (0, 2):
                B = len(rots)
                out.append(dict(table=table, name="%s-mode%d-%s" % (table, mode, ds), dataset=ds, npoints=8, R=64,
                                lengths=[[64, 61]] * B, survivors=[(ex, ex)] * B, step=1, seed=SEED, device_lengths=False,
                                mode=mode, rotations=[r for _n, r, _x in rots], names=[n for n, _r, _x in rots]))
    return out


def wide_cases():
    """B = 257, R = 64, npoints = 8: mode 1 (drawn) and 2 (given) for KITTI-360, mode 2 for KITTI."""
    ex = ("except", 5, 1)
    B = 257
    return [dict(table="wide", name="wide-mode%d-%s" % (mode, ds), dataset=ds, npoints=8, R=64, lengths=[[64, 64 - b % 5] for b in range(B)],
                 survivors=[(ex, ex)] * B, step=4, seed=SEED, device_lengths=False, mode=mode)
            for ds, mode in (("kitti360", 1), ("kitti360", 2), ("kitti", 2))]


def all_cases():
    return selection_cases() + pose_cases() + wide_cases()


# ---- arrays -----------------------------------------------------------------------------------------------------------------
def keeps(case):
    """(B, 2, R) bool: the rows made to survive."""
    return np.stack([np.stack([keep_mask(sv[f], case["R"]) for f in range(2)]) for sv in case["survivors"]])


def materialise(case):
    """-> dict(sweeps (B,2,R,4) f32, lengths (B,2) int64, t_diff (B,4,4) f64, aug (B,6) f32 or None, tr, keep (B,2,R))."""
    B, R = len(case["lengths"]), case["R"]
    keep = keeps(case)
    sweeps = np.stack([np.stack([raw_rows(R, 2 * b + f) for f in range(2)]) for b in range(B)])
    sweeps[..., 0][~keep] = 100.0
    t_diff = motions(B)
    if "rotations" in case:
        for b, r in enumerate(case["rotations"]):
            t_diff[b, :3, :3] = r
            t_diff[b, :3, 3] = POSE_TRANSLATION
    return dict(sweeps=sweeps, lengths=np.array(case["lengths"], dtype=np.int64), t_diff=t_diff,
                aug=given_params(B) if case["mode"] == 2 else None, tr=VELO_TO_CAM if case["dataset"] == "kitti" else None,
                keep=keep)


def expected(case, arrays, aug=None, fault=None):
    """The host model's batch for a case; ``aug`` replaces the parameters (the device's own drawn ones, for mode 1)."""
    if aug is None:
        aug = arrays["aug"]
    return model.build(case["dataset"], arrays["sweeps"], arrays["lengths"], arrays["t_diff"], case["npoints"], case["seed"],
                       case["step"], augment=case["mode"] != 0, aug=aug, tr=arrays["tr"],
                       clamp_lengths=case["device_lengths"], fault=fault)
