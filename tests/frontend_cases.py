"""The case tables of tests/test_gpu_frontend.py with their inputs, shared with tests/test_frontend_cases_cpu.py, which proves
that the tables reach every class of the kernels' own arithmetic and tell the host model (tests/frontend_model.py) from
each of its planted faults.  CPU NumPy only.

Filters.  Three calibrations: "general" (a KITTI-like Tr with translation), "permute" (x' = y, y' = z, z' = x, zero
translation: every output IS an input, so a row can sit exactly on +-30 and on the fp32 neighbours either side) and "scale"
(the permutation with y' = 1.1 z: z = 1 gives the float64 1.1 itself, which no fp32 input reaches under "permute" -- the only
way to tell ``y' > 1.1`` from ``>=``).  ``filter_rows`` puts the threshold rows and NaN, +-Inf, -0.0 and both signs of the
smallest subnormal in every column at the head of a frame; random rows follow.  n in FILTER_N, and one (3, 257, 4) batch.

Compaction.  Both compaction kernels give wave w of 16 the rows [w per_wave, (w + 1) per_wave), per_wave = the rows per wave
rounded up to 64, and walk a range 64 rows at a time.  ``layout_class(n)`` = (per_wave, how many ranges are non-empty: "one" /
"some" / "all", how full the last 64-step is: "single" row / "short" / "full"); COMPACT_N holds the lengths the issue names
and one more for every class a frame of up to 2049 rows can have.  Seven keep patterns (a different one per frame), kept
rows marked with the words 1, 2, -1 and INT_MIN in turn, caps around each frame's count, and the two fills of
tests/gather_cases.py ("identity": the fp32 integer of the source row and column; "bits": NaN payloads, -0.0, subnormals).

Sweeps.  S = 4 streams per launch over one (4, SWEEP_R, 4) buffer: every length of COMPACT_N, 0, -5 and SWEEP_R + 9.
"""
import numpy as np

import frontend_model as FM
import gather_cases as GC

SENTINEL = GC.SENTINEL
INT_MIN = -2 ** 31
KEEP_WORDS = np.array([1, 2, -1, INT_MIN], dtype=np.int64).astype(np.int32)
F32 = np.float32


def _nb(v, up):
    return np.nextafter(F32(v), F32(np.inf if up else -np.inf))


# ---- filters --------------------------------------------------------------------------------------------------------------
GENERAL_TR = np.array([[4.3e-4, -0.99997, -8.0e-3, -1.2e-2], [-7.2e-3, 8.1e-3, -0.99994, -5.4e-2],
                       [0.99997, 4.9e-4, -7.2e-3, -0.292]])
PERMUTE_TR = np.array([[0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 0.0]])
SCALE_TR = np.array([[0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.1, 0.0], [1.0, 0.0, 0.0, 0.0]])
CALIBRATIONS = {"general": GENERAL_TR, "permute": PERMUTE_TR, "scale": SCALE_TR}
NEAR = 30.0
GROUND_Z = FM.KITTI360_GROUND_Z
FILTER_N = (1, 255, 256, 257)
FILTER_BATCH = (3, 257)
SPECIAL_VALUES = np.array([0x7FC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x80000001],
                          dtype=np.uint32).view(np.float32)      # NaN, +Inf, -Inf, -0.0, +-smallest subnormal


def _threshold_rows(dataset):
    """Rows in OUTPUT space (x', y', z') for "kitti" (read through the permutation), in input space for "kitti360"."""
    base = np.array([1.0, 0.5, 2.0], dtype=F32)                  # kept by both filters
    rows = []

    def put(col, v):
        r = base.copy()
        r[col] = v
        rows.append(r)
    if dataset == "kitti":
        for col in (0, 2):
            for t in (NEAR, -NEAR):
                for v in (_nb(t, False), F32(t), _nb(t, True)):
                    put(col, v)
        lo = F32(1.1) if F32(1.1) < 1.1 else _nb(1.1, False)     # the two fp32 neighbours of the float64 1.1
        put(1, lo)
        put(1, _nb(lo, True))
    else:
        gz = F32(GROUND_Z)
        for v in (_nb(gz, False), gz, _nb(gz, True)):
            put(2, v)
        for col in (0, 1):
            for t in (NEAR, -NEAR):
                for v in (_nb(t, False), F32(t), _nb(t, True)):
                    put(col, v)
    return np.stack(rows)


def filter_rows(dataset, calib="permute"):
    """(m, 4) f32 raw rows: thresholds, then every special value in every column of a row that is kept otherwise."""
    thr = _threshold_rows(dataset)
    if dataset == "kitti":
        thr = thr[:, [2, 0, 1]]                                  # x = z', y = x', z = y'
        if calib == "scale":
            thr[:, 2] = np.where(np.arange(len(thr)) % 2 == 0, F32(1.0), thr[:, 2])    # y' = 1.1 z = the float64 1.1
    rows = [np.append(r, F32(0.25)) for r in thr]
    base = np.array([2.0, 1.0, 0.5, 0.25], dtype=F32)            # x' = 1, y' = .5, z' = 2 / kept by kitti360 as well
    for col in range(4):
        for v in SPECIAL_VALUES:
            r = base.copy()
            r[col] = v
            rows.append(r)
    return np.stack(rows).astype(F32)


def filter_frame(dataset, calib, n, seed):
    """(n, 4) f32: ``filter_rows`` first (as many as fit), then random rows around the thresholds."""
    rng = np.random.default_rng(seed)
    pts = np.concatenate([rng.uniform(-45, 45, (n, 2)), rng.uniform(-3, 3, (n, 1)), rng.uniform(0, 1, (n, 1))],
                         axis=1).astype(F32)
    head = filter_rows(dataset, calib)
    m = min(n, len(head))
    pts[:m] = head[:m]
    return pts


def filter_cases():
    """[(dataset, calib or None, shape)]: every n with every calibration, and the batch."""
    out = []
    for shape in [(n,) for n in FILTER_N] + [FILTER_BATCH]:
        out += [("kitti", c, shape) for c in CALIBRATIONS] + [("kitti360", None, shape)]
    return out


def filter_input(case):
    dataset, calib, shape = case
    n = int(np.prod(shape))
    seed = 1000 * n + 7 * len(shape) + (0 if calib is None else 1 + sorted(CALIBRATIONS).index(calib))
    if len(shape) == 1:
        return filter_frame(dataset, calib, n, seed)
    frames = [filter_frame(dataset, calib, shape[1], seed + f) for f in range(shape[0])]
    for f in range(1, shape[0]):                                 # the special rows at another place in every frame
        frames[f] = np.roll(frames[f], 100 * f, axis=0)
    return np.stack(frames)


def filter_model(case, pts, fault=None):
    dataset, calib, _ = case
    if dataset == "kitti":
        return FM.kitti_row(pts.reshape(-1, 4), CALIBRATIONS[calib], fault)
    return FM.kitti360_row(pts.reshape(-1, 4), GROUND_Z, NEAR, fault)


# ---- compaction -----------------------------------------------------------------------------------------------------------
ISSUE_N = (1, 63, 64, 65, 1023, 1024, 1025, 2047, 2049)
COMPACT_N = ISSUE_N + (100, 128, 961, 1100, 1152, 1921, 2048)
COMPACT_B = (1, 3)
PATTERNS = ("all", "none", "first", "last", "alternating", "one_per_wave", "bernoulli")
MAX_N = 2049


def layout_class(n):
    per_wave, ranges = FM.wave_layout(n)
    live = sum(1 for i0, i1 in ranges if i0 < i1)
    return (per_wave, "one" if live == 1 else ("all" if live == 16 else "some"),
            "single" if n % 64 == 1 else ("full" if n % 64 == 0 else "short"))


def keep_pattern(name, n, seed):
    """(n,) int32: 0 for a dropped row, one of KEEP_WORDS (in turn along the kept rows) for a kept one."""
    k = np.zeros(n, dtype=bool)
    if name == "all":
        k[:] = True
    elif name == "first":
        k[0] = True
    elif name == "last":
        k[n - 1] = True
    elif name == "alternating":
        k[1::2] = True
        k[0] = n == 1
    elif name == "one_per_wave":
        for w, (i0, i1) in enumerate(FM.wave_layout(n)[1]):
            if i0 < i1:
                k[i0 + (37 * w + 5) % (i1 - i0)] = True
    elif name == "bernoulli":
        k = np.random.default_rng(seed).random(n) < 0.3
    else:
        assert name == "none"
    out = np.zeros(n, dtype=np.int32)
    idx = np.nonzero(k)[0]
    out[idx] = KEEP_WORDS[np.arange(len(idx)) % 4]
    return out


def frame_patterns(pattern, b):
    """The pattern of every frame of a batch: a different one per frame."""
    at = PATTERNS.index(pattern)
    return [PATTERNS[(at + 3 * f) % len(PATTERNS)] for f in range(b)]


def compact_keep(pattern, b, n):
    return np.stack([keep_pattern(p, n, 97 * n + f) for f, p in enumerate(frame_patterns(pattern, b))])


def caps_for(counts, n):
    """cap in {1, count - 1, count, count + 1, n, n + 7} for every frame's (unclipped) count, positive ones, ascending."""
    caps = {1, n, n + 7}
    for c in counts:
        caps |= {c - 1, c, c + 1}
    return sorted(c for c in caps if c >= 1)


def xyz_fill(kind, b, n, seed):
    """(b, n, 3) int32 words.  "identity": the fp32 integer (f n + i) 3 + column; "bits": gather_cases.fill_bits."""
    return GC.fill(kind, b, n, 3, seed)


def compact_cases():
    """[(n, b, pattern, fill)] -- the caps follow from the counts (``caps_for``)."""
    return [(n, b, p, fill) for n in COMPACT_N for b in COMPACT_B for p in PATTERNS for fill in GC.FILLS]


def guard_buffer(cap, guard, word=SENTINEL):
    return np.full((cap + guard, 3), word, dtype=np.int32)


# ---- sweeps ---------------------------------------------------------------------------------------------------------------
SWEEP_R = 2060
SWEEP_S = 4
SWEEP_LENGTHS = ((1, 63, 64, 65), (1023, 1024, 1025, 100), (2047, 2049, 0, 128), (-5, SWEEP_R + 9, 961, 2048),
                 (1100, 1152, 1921, SWEEP_R))
LONG_THEN_SHORT = ((2049, SWEEP_R, 1025, 2047), (3, 0, 1024, 65))
SWEEP_PREFILL = F32(7.0).view(np.int32)
DATASETS = ("kitti", "kitti360")
TAILS = ("nan", "live")


def sweep_trs():
    """(4, 12) float64: a calibration per stream -- the general one, a perturbed copy, the permutation and "scale"."""
    rng = np.random.default_rng(5)
    return np.stack([GENERAL_TR, GENERAL_TR + rng.normal(0, 1e-3, (3, 4)), PERMUTE_TR, SCALE_TR]).reshape(4, 12)


SWEEP_CALIBS = ("general", "general", "permute", "scale")      # whose threshold rows head every stream's frame


def sweep_batch(dataset, lengths, tail, seed):
    """(4, SWEEP_R, 4) f32: stream s holds a filter frame; rows past its (clamped) length are NaN ("nan") or stay the
    frame's own rows, which a kernel that read on would keep some of ("live")."""
    out = np.empty((SWEEP_S, SWEEP_R, 4), dtype=F32)
    for s, L in enumerate(lengths):
        out[s] = filter_frame(dataset, SWEEP_CALIBS[s], SWEEP_R, seed + s)
        if tail == "nan":
            out[s, min(max(L, 0), SWEEP_R):] = np.nan
    return out


def sweep_model(dataset, batch, lengths, cap, buffers, fault=None):
    """Every stream through the model on its own buffer -> ([buffer after], [count])."""
    trs = sweep_trs()
    res = [FM.sweep_filter_compact(batch, s, L, cap, buffers[s], dataset, tr=trs[s], ground_z=GROUND_Z, near=NEAR, fault=fault)
           for s, L in enumerate(lengths)]
    return [r[0] for r in res], [r[1] for r in res]


def sweep_counts(dataset, batch, lengths):
    """The unclipped survivor counts of a launch (what the caps are placed around)."""
    big = [guard_buffer(SWEEP_R, 1) for _ in lengths]
    return sweep_model(dataset, batch, lengths, SWEEP_R, big)[1]


# ---- ingest ---------------------------------------------------------------------------------------------------------------
INGEST_N = (1, 255, 256, 257)
INGEST_B = (1, 2)
INGEST_T = (1, 3)
INGEST_C = (3, 4, 5)
INGEST_EXTRA = (0, 3)                  # n_total - n
