"""Named edge cases of the loop detector's kernels, one rule deciding each, shared by
tests/test_loop_closure_edges_cpu.py (which proves on the model that every case takes the branch it is named after) and
tests/test_gpu_loop_closure_edges.py (which runs each kernel alone on them).  Masks, descriptors, scores and words are
planted, not derived from clouds.  A case is a dict with ``kind``, ``name``, the inputs of one stream and ``want``, the fields
of the model's answer that the rule fixes.  ``prior_cases()`` restates the inputs of the GPU files that existed before."""
import numpy as np

import loop_closure_cases as C
import loop_closure_model as M

F = np.float32
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
SHAPES = list(C.SHAPES) + [(2, 63), (64, 8), (1, 64)]
COUNT_MK = [(c, c + d) for c in (1, 3, 4, 5) for d in (0, 1)]        # MK = 1, 2, 3, 4, 5, 6: mostly no multiple of four
MIN_ID = 10
THRESHOLD = 0.2


def signed(mask):
    """A 64-bit mask as the int64 torch holds."""
    return mask - (1 << 64) if mask >> 63 else mask


def planted(rng, NR, NS, mask):
    """A normalised descriptor whose non-empty columns are exactly the bits of ``mask``."""
    D = np.zeros((NR, NS), dtype=F)
    cols = [j for j in range(NS) if mask >> j & 1]
    D[:, cols] = rng.uniform(0.1, 3.0, (NR, len(cols))).astype(F)
    Dn, m = M.normalise(D)
    assert m == mask
    return Dn


def seen(Q, s):
    """The place a query Q sees ``s`` sectors further round: E[:, j] = Q[:, (j + s) mod NS]."""
    return np.roll(Q, -s, axis=1)


# ---- search: the score kernel --------------------------------------------------------------------------------------------------

def search_cases():
    out = []
    for si, (NR, NS) in enumerate(SHAPES):
        full = (1 << NS) - 1
        rng = np.random.default_rng(1000 + si)
        turn = [si]

        def add(name, Qn, qmask, special, smask, want, need=1):
            while COUNT_MK[turn[0] % 8][0] < max(need, len(special)):
                turn[0] += 1
            count, MK = COUNT_MK[turn[0] % 8]
            turn[0] += 1
            fill = count - len(special)
            En = [planted(rng, NR, NS, full) for _ in range(fill)] + list(special)
            em = [full] * fill + list(smask)
            want = dict(want)
            for key in ("entry", "at"):                      # positions are given among the specials: they sit last
                if want.get(key, -1) is not None and want.get(key, -1) >= 0:
                    want[key] += fill
            tie = want.pop("tie", False) or NR == 1          # one ring: every non-empty column is the number 1
            out.append(dict(kind="search", name="%s-%dx%d-c%d-mk%d" % (name, NR, NS, count, MK), rule=name, NR=NR, NS=NS,
                            MK=MK, count=count, Qn=np.asarray(Qn, dtype=F), qmask=qmask, En=np.stack(En).astype(F), emask=em,
                            frame_ids=np.arange(count, dtype=np.int32) * 2, f=2 * count + 50, min_id=MIN_ID, positions=None,
                            max_distance=None, active=1, want=want, tie=tie))

        Q = planted(rng, NR, NS, full)
        s = NS // 3
        noisy = seen(Q, s) + rng.uniform(0.0, 0.02, (NR, NS)).astype(F)
        add("full", Q, full, [M.normalise(noisy)[0]], [full], dict(entry=0, shift=s))
        col = planted(rng, NR, NS, 1)
        k = NS // 2
        add("bit0_one_overlap", col, 1, [seen(col, NS - k)], [1 << k], dict(entry=0, shift=NS - k, overlaps=1))
        last = planted(rng, NR, NS, 1 << (NS - 1))
        add("bit_last_to_bit0", last, 1 << (NS - 1), [seen(last, NS - 1)], [1], dict(entry=0, shift=NS - 1, overlaps=1))
        add("bit_last_same", last, 1 << (NS - 1), [last], [1 << (NS - 1)], dict(entry=0, shift=0, overlaps=1))
        add("query_mask0", np.zeros((NR, NS), dtype=F), 0, [], [], dict(entry=-1, all_inf=True), need=3)
        add("entry_mask0", Q, full, [np.zeros((NR, NS), dtype=F), Q], [0, full], dict(at=0, inf_at=True, entry=1, shift=0),
            need=3)
        outside = ((1 << 64) - 1) ^ full                   # no bit inside [0, NS): disjoint from the query at every shift
        add("disjoint", Q, full, [Q, seen(Q, 1)], [outside, full], dict(at=0, inf_at=True, entry=1, shift=1), need=3)
        add("last_shift", Q, full, [seen(Q, NS - 1)], [full], dict(entry=0, shift=NS - 1))
        if NS % 2 == 0:
            half = planted(rng, NR, NS // 2, (1 << (NS // 2)) - 1)
            P = M.normalise(np.concatenate([half, half], axis=1))[0]
            s0 = NS // 2 - 1
            add("period", P, full, [seen(P, s0)], [full], dict(entry=0, shift=s0, tie=True, tied_shift=s0 + NS // 2))
        add("equal", Q, full, [Q], [full], dict(entry=0, shift=0))
        add("equal_twice", Q, full, [Q, Q], [full, full], dict(entry=0, shift=0, tie=True, tied_entry=1), need=3)
    return out


GATE_FRAMES = 31


def gate_cases():
    """The eligibility rules, at (20, 60) with three places: the id rule, the distance gate and the guards of both reads."""
    NR, NS, count, MK = 20, 60, 3, 4
    full = (1 << NS) - 1
    rng = np.random.default_rng(77)
    Q = planted(rng, NR, NS, full)
    En = np.stack([seen(Q, 3), seen(Q, 5), seen(Q, 7)])
    nan = np.nan
    out = []

    def add(name, ids, f, ok, min_id=5, max_distance=5.0, where=None, group="gate"):
        pos = np.zeros((GATE_FRAMES, 3))
        for frame, p in (where or {}).items():
            pos[frame] = p
        out.append(dict(kind="search", name="gate_" + name, rule="gate_" + name, NR=NR, NS=NS, MK=MK, count=count, Qn=Q,
                        qmask=full, En=En, emask=[full] * 3, frame_ids=np.array(ids, dtype=np.int32), f=f, min_id=min_id,
                        positions=pos, max_distance=max_distance, active=1, want=dict(eligible=ok), tie=False, group=group))

    add("distance_equal", [0, 1, 2], 30, [0, 1, 1], where={0: (3.0, 4.0, 0.0)})            # d2 == max_distance^2: out
    add("distance_below", [0, 1, 2], 30, [1, 1, 1], where={0: (3.0, np.nextafter(4.0, 0.0), 0.0)})
    add("id_equal", [24, 25, 26], 30, [1, 1, 0])                                           # fe + min_id == f counts
    add("f_is_frames", [0, 1, 2], GATE_FRAMES, [0, 0, 0])
    add("f_negative", [-20, -19, -18], -1, [0, 0, 0])
    add("entry_is_frames", [GATE_FRAMES, 0, 1], GATE_FRAMES + 5, [0, 0, 0])                # both lie outside: see the README
    add("entry_minus_one", [-1, 0, 1], 30, [0, 1, 1])
    add("nan_query_position", [0, 1, 2], 30, [0, 0, 0], where={30: (nan, 0.0, 0.0)})
    add("nan_entry_position", [0, 1, 2], 30, [1, 0, 1], where={1: (0.0, nan, 0.0)})
    add("same_frame", [30, 29, 31], 30, [1, 1, 0], min_id=0, group="gate0")                 # min_id_distance = 0: fe == f
    return out


# ---- select on planted scores --------------------------------------------------------------------------------------------------

SELECT_MK = (1, 255, 256, 257, 513, 1025)
SELECT_NS = 60


def select_cases():
    out = []
    below = np.nextafter(F(THRESHOLD), F(0))
    for MK in SELECT_MK:
        rng = np.random.default_rng(MK)

        def add(name, plant, want, threshold=THRESHOLD, stride=1, count=None, active=1, f=7, base=None):
            sc = rng.uniform(0.3, 1.0, MK).astype(F) if base is None else np.full(MK, base, dtype=F)
            for at, v in plant.items():
                sc[at] = v
            cnt = MK if count is None else count
            if cnt < MK:
                sc[max(cnt, 0):] = np.inf                    # as the score kernel leaves the entries past the count
            out.append(dict(kind="select", name="%s-mk%d" % (name, MK), rule=name, MK=MK, NS=SELECT_NS, scores=sc,
                            shifts=rng.integers(0, SELECT_NS, MK).astype(np.int32),
                            frame_ids=rng.integers(0, 1000, MK).astype(np.int32), count=cnt, active=active, f=f, stride=stride,
                            threshold=threshold, want=want))

        add("min_last", {MK - 1: 0.05}, dict(entry=MK - 1, found=1, slot=-1, overflow=True))
        if MK > 256:
            i = MK - 257
            add("tie_stride", {i: 0.05, i + 256: 0.05}, dict(entry=i, found=1))
        if MK > 257:
            add("tie_2_257", {2: 0.05, 257: 0.05}, dict(entry=2, found=1))     # the lower entry sits in the higher thread
        if MK > 300:
            add("tie_10_300", {10: 0.05, 300: 0.05}, dict(entry=10, found=1))
        if MK > 1:
            add("nan_first", {0: np.nan, 1: 0.05}, dict(entry=1, found=1))
            add("zero_signs", {MK // 2: 0.0, MK - 1: -0.0}, dict(entry=MK // 2, found=1, score_bits=0))
            add("zero_signs_reversed", {MK // 2: -0.0, MK - 1: 0.0}, dict(entry=MK // 2, found=1, score_bits=INT_MIN))
            add("short_count", {0: 0.05}, dict(entry=0, found=1, slot=MK - 1, overflow=False), count=MK - 1)
        add("nan_all", {}, dict(entry=-1, found=0, score_bits=0x7F800000), base=np.nan)
        add("inf_all", {}, dict(entry=-1, found=0, score_bits=0x7F800000), base=np.inf)
        add("neg_inf", {MK // 2: -np.inf}, dict(entry=MK // 2, found=1))
        add("at_threshold", {MK // 3: F(THRESHOLD)}, dict(entry=MK // 3, found=0))
        add("below_threshold", {MK // 3: below}, dict(entry=MK // 3, found=1))
        add("threshold_inf", {0: 3.0e38}, dict(entry=0, found=1), threshold=np.inf, base=np.inf)
        add("threshold_negative", {0: 0.0}, dict(entry=0, found=0), threshold=-0.5)
        add("threshold_negative_hit", {0: -1.0}, dict(entry=0, found=1), threshold=-0.5)
        # the slot: -1 for each of these, overflow only for a full database
        add("slot_f_minus_one", {}, dict(slot=-1, overflow=False), f=-1, count=0)
        add("slot_f_int_min", {}, dict(slot=-1, overflow=False), f=INT_MIN, count=0, stride=2)
        add("slot_f_minus_two", {}, dict(slot=-1, overflow=False), f=-2, count=0, stride=2)
        add("slot_off_stride", {}, dict(slot=-1, overflow=False), f=7, count=0, stride=2)
        add("slot_on_stride", {}, dict(slot=0, overflow=False), f=8, count=0, stride=2)
        add("slot_full", {}, dict(slot=-1, overflow=True), count=MK)
        add("slot_past_full", {}, dict(slot=-1, overflow=True), count=MK + 3)
        add("slot_full_off_stride", {}, dict(slot=-1, overflow=False), f=7, count=MK, stride=2)
        add("slot_inactive", {0: 0.05}, dict(entry=-1, found=0, slot=-1, overflow=False, score_bits=0x7F800000), active=0,
            count=MK)
    return out


# ---- accept --------------------------------------------------------------------------------------------------------------------

ACCEPT_S = (1, 64, 65, 130)


def product_off_an_integer():
    """A (min_fitness, n) whose fp64 product is no integer though the decimal one is: found by search."""
    for tenths in range(1, 10):
        mf = tenths / 10.0
        for n in range(64, 4096):
            p = mf * n
            if p != np.floor(p) and (tenths * n) % 10 == 0:
                return mf, n, tenths * n // 10
    raise AssertionError("no such product")


def accept_tables():
    """-> list of (config name, dict(n, min_fitness, max_mean_cost, ML, status: False for ``status=None``), rows); a row is
    dict(name, found, status, pairs, cost, nlog, want)."""
    nan, inf = np.nan, np.inf
    row = lambda name, want, found=1, status=0, pairs=32, cost=0.5, nlog=0: dict(
        name=name, found=found, status=status, pairs=pairs, cost=cost, nlog=nlog, want=want)
    main = [row("not_found", 0, found=0), row("few_pairs", 0, status=2), row("bad_pivot", 0, status=4),
            row("both_bits", 0, status=6), row("bit_1", 1, status=1), row("bit_8", 1, status=8), row("bits_1_8", 1, status=9),
            row("pairs_15", 0, pairs=15, cost=0.1), row("pairs_16", 1, pairs=16, cost=0.1),
            row("mean_at_bound", 1, pairs=16, cost=1.0), row("mean_above", 0, pairs=16, cost=np.nextafter(1.0, 2.0)),
            row("cost_nan", 0, cost=nan), row("cost_negative", 1, cost=-3.0), row("cost_neg_inf", 1, cost=-inf),
            row("pairs_0", 0, pairs=0, cost=0.0), row("pairs_negative", 0, pairs=-5, cost=-1.0),
            row("pairs_int_max", 1, pairs=INT_MAX, cost=1.0),
            row("log_empty", 1, nlog=0), row("log_last_row", 1, nlog=3), row("log_full", "overflow", nlog=4),
            row("log_past_full", "overflow", nlog=5), row("log_full_refused", 0, nlog=4, status=2)]
    mf, n, whole = product_off_an_integer()
    side = int(np.floor(mf * n)), int(np.floor(mf * n)) + 1
    zero = [row("quotient_nan", None, pairs=0, cost=0.0), row("quotient_inf", None, pairs=0, cost=2.0),
            row("quotient_minus_inf", None, pairs=0, cost=-2.0)]
    small = [row("log_empty", 1, nlog=0), row("log_full", "overflow", nlog=1), row("log_past_full", "overflow", nlog=2)]
    return [
        ("main", dict(n=64, min_fitness=0.25, max_mean_cost=0.0625, ML=4, status=True), main),
        ("one_double_lower", dict(n=64, min_fitness=0.25, max_mean_cost=float(np.nextafter(0.0625, 0.0)), ML=4, status=True),
         [row("mean_at_old_bound", 0, pairs=16, cost=1.0), row("mean_below", 1, pairs=16, cost=np.nextafter(1.0, 0.0))]),
        ("product", dict(n=n, min_fitness=mf, max_mean_cost=1.0, ML=4, status=True),
         [row("below_product", 0, pairs=side[0], cost=0.0), row("above_product", 1, pairs=side[1], cost=0.0)]),
        ("no_pairs", dict(n=64, min_fitness=0.0, max_mean_cost=0.0625, ML=4, status=True),
         [dict(zero[0], want=0), dict(zero[1], want=0), dict(zero[2], want=1)]),            # -inf <= any bound
        # pinned, not required beforehand: NaN <= inf is false, inf <= inf true, -inf <= inf true
        ("no_pairs_any_cost", dict(n=64, min_fitness=0.0, max_mean_cost=float("inf"), ML=4, status=True),
         [dict(zero[0], want=0), dict(zero[1], want=1), dict(zero[2], want=1)]),
        ("one_row_log", dict(n=64, min_fitness=0.25, max_mean_cost=0.0625, ML=1, status=True), small),
        ("no_status", dict(n=64, min_fitness=0.0, max_mean_cost=0.0, ML=4, status=False),
         [row("logged", 1, status=6, pairs=3, cost=9.0), row("not_found", 0, found=0), row("log_full", "overflow", nlog=4)]),
    ]


def accept_streams(rows, S, seed=0):
    """One case per stream, cycling through the table: the per-stream inputs of one launch."""
    rng = np.random.default_rng(seed + S)
    pick = [rows[s % len(rows)] for s in range(S)]
    return dict(rows=pick, found=np.array([r["found"] for r in pick], dtype=np.int32),
                match=np.stack([[r["found"], s % 5, 100 + s, s % 60] for s, r in enumerate(pick)]).astype(np.int32),
                score=rng.uniform(0.0, 0.2, S).astype(F), f=(500 + np.arange(S)).astype(np.int32), T=rng.normal(size=(S, 4, 4)),
                status=np.array([r["status"] for r in pick], dtype=np.int32),
                pairs=np.array([r["pairs"] for r in pick], dtype=np.int32),
                cost=np.array([r["cost"] for r in pick], dtype=np.float64),
                nlog=np.array([r["nlog"] for r in pick], dtype=np.int32))


# ---- fetch and insert ----------------------------------------------------------------------------------------------------------

COPY_MK = 3
COPY_N = (1, 682, 683, 1366)                             # 3 n = 3, 2046, 2049, 4098 around the grid stride of 2048 floats
COPY_SHAPES = ((1, 8), (20, 60), (3, 63), (64, 64))      # 64 x 64 = 4096 cells: the cell loop takes two trips


def payload(rng, n):
    """A cloud whose rows carry NaN payloads, infinities and -0.0: copied as words, never as numbers."""
    c = rng.normal(size=(n, 3)).astype(F)
    raw = c.view(np.int32).reshape(-1)
    raw[0::7] = 0x7FC0BEEF - np.arange(len(raw[0::7]), dtype=np.int32)        # NaNs, each with its own payload
    raw[1::11] = INT_MIN                                                      # -0.0
    return raw.view(F).reshape(n, 3)


def fetch_rows():
    MK = COPY_MK
    return [dict(name="not_found", found=0, entry=1, want=False), dict(name="entry_minus_one", found=1, entry=-1, want=False),
            dict(name="entry_is_MK", found=1, entry=MK, want=False), dict(name="entry_last", found=1, entry=MK - 1, want=True),
            dict(name="entry_first", found=1, entry=0, want=True), dict(name="entry_int_min", found=1, entry=INT_MIN, want=False),
            dict(name="not_found_bad_entry", found=0, entry=MK + 7, want=False)]


def insert_rows():
    MK = COPY_MK
    bit63 = 1 << 63
    return [dict(name="slot_minus_one", slot=-1, count=2, mask=5, want=False), dict(name="slot_is_MK", slot=MK, count=MK, mask=5, want=False),
            dict(name="slot_last", slot=MK - 1, count=MK - 1, mask=bit63 | 1, want=True),
            dict(name="slot_first", slot=0, count=0, mask=bit63, want=True),
            dict(name="count_ignored", slot=1, count=-7, mask=(1 << 64) - 1, want=True),
            dict(name="count_ahead", slot=0, count=MK, mask=0, want=True),
            dict(name="slot_int_min", slot=INT_MIN, count=1, mask=5, want=False)]


def fetch_streams(n):
    """One stream per row of ``fetch_rows`` -> dict(rows, found (S,), match (S, 4), db_cloud (S, MK, n, 3))."""
    rows = fetch_rows()
    rng = np.random.default_rng(n)
    return dict(rows=rows, found=np.array([r["found"] for r in rows], dtype=np.int32),
                match=np.array([[r["found"], r["entry"], 9, 3] for r in rows], dtype=np.int32),
                db_cloud=np.stack([np.stack([payload(rng, n) for _ in range(COPY_MK)]) for _ in rows]))


def insert_streams(n, NR, NS):
    """One stream per row of ``insert_rows`` -> dict(rows, slot, f, count, Qn (S, NR, NS), qmask (python ints), cloud)."""
    rows = insert_rows()
    rng = np.random.default_rng(n + NS)
    Qn = rng.normal(size=(len(rows), NR, NS)).astype(F)
    Qn.view(np.int32).reshape(len(rows), -1)[:, 0] = 0x7FC00123          # a NaN payload in a descriptor word
    return dict(rows=rows, slot=np.array([r["slot"] for r in rows], dtype=np.int32),
                f=(40 + np.arange(len(rows))).astype(np.int32), count=np.array([r["count"] for r in rows], dtype=np.int32),
                Qn=Qn, qmask=[r["mask"] for r in rows], cloud=np.stack([payload(rng, n) for _ in rows]))


# ---- build ---------------------------------------------------------------------------------------------------------------------

BUILD_N = (1, 255, 256, 257)


def build_streams(n, rings=20, sectors=60):
    """The streams of one build launch at ``n`` points: the nine (active, restart) pairs with the lengths cycling, then the
    planted clouds.  -> list of dict(name, cloud, length, active, restart, z_offset), all at z_offset 2."""
    rng = np.random.default_rng(n)
    lengths = [INT_MIN, -1, 0, n, n + 1]
    out = []
    k = 0
    for active in (0, 1, 2):
        for restart in (0, 1, 2):
            cloud = C.pad(C.cell_centres(n + k, rings, sectors), n, seed=k)
            out.append(dict(name="words_a%d_r%d" % (active, restart), cloud=cloud, length=lengths[k % 5], active=active,
                            restart=restart))
            k += 1
    for length in lengths:
        out.append(dict(name="length_%d" % length, cloud=C.pad(C.cell_centres(n + 50, rings, sectors), n, seed=3),
                        length=length, active=1, restart=0))
    dropped = np.zeros((n, 3), dtype=F)
    dropped[:, 0], dropped[:, 2] = 100.0 + np.arange(n), 1.0                    # beyond max_range
    dropped[::3] = (1.0, 1.0, -5.0)                                             # below the ground
    dropped[1::5] = (0.0, 0.0, 1.0)                                             # r2 == 0
    dropped[2::7] = (np.nan, 1.0, 1.0)
    out.append(dict(name="all_dropped", cloud=dropped, length=n, active=1, restart=0))
    cell = np.zeros((n, 3), dtype=F)
    cell[:, 0], cell[:, 1] = 11.0 + rng.uniform(0, 0.5, n), 3.0 + rng.uniform(0, 0.1, n)
    cell[:, 2] = rng.uniform(-1.0, 3.0, n)
    out.append(dict(name="one_cell", cloud=cell, length=n, active=1, restart=0))
    huge = cell.copy()
    huge[0, 2] = 2.0e19                                                         # its square overflows: norm inf, Dn 0
    out.append(dict(name="height_overflows", cloud=huge, length=n, active=1, restart=0))
    ground = cell.copy()
    ground[:, 2] = -2.0                                                         # h == 0 exactly: dropped
    ground[0, 2] = np.nextafter(F(-2.0), F(0))                                  # one ulp above: kept, h = 2^-23
    out.append(dict(name="height_zero_and_beside", cloud=ground, length=n, active=1, restart=0))
    return out


TINY = float(np.float32(2.0 ** -126))                    # the smallest normal float as z_offset


def tiny_streams(n):
    """z_offset = 2^-126.  fp32 addition never rounds a non-zero sum to 0 (gradual underflow), so "z + z_offset rounds to 0"
    is the exact 0 (dropped) and its neighbour is the smallest subnormal (kept; a flushing adder would drop it)."""
    base = np.zeros((n, 3), dtype=F)
    base[:, 0], base[:, 1] = 11.0, 3.0
    zero, sub, below = base.copy(), base.copy(), base.copy()
    zero[:, 2] = -F(TINY)
    sub[:, 2] = -F(TINY)
    sub[0, 2] = np.nextafter(-F(TINY), F(0))                                    # h = 2^-149
    below[:, 2] = np.nextafter(-F(TINY), F(-1))                                 # h = -2^-149
    plain = base.copy()
    plain[:, 2] = F(2.0 ** -140)                                                # a subnormal z: h is normal
    return [dict(name="sum_zero", cloud=zero, length=n, active=1, restart=0),
            dict(name="sum_subnormal", cloud=sub, length=n, active=1, restart=0),
            dict(name="sum_below_zero", cloud=below, length=n, active=1, restart=0),
            dict(name="subnormal_z", cloud=plain, length=n, active=1, restart=0)]


# ---- what the files before this one ran ----------------------------------------------------------------------------------------

def prior_cases():
    """The inputs of tests/test_gpu_loop_closure.py and of the whole-chain scenes, in this file's format, so that the planted
    faults can be run over them: the five search cases (forwards, reversed and empty), the rule table of test_search_rules,
    the select and slot words those launches saw, and the accept and insert calls of the scenes (pairs and costs as DESIGN.md
    section 26 records them)."""
    out = []
    rings, sectors = C.SEARCH_SHAPE
    for count in C.SEARCH_COUNTS:
        c = C.search_case(count)
        _, Qn, qmask = M.descriptor(c["query"], rings, sectors)
        for name, order in (("forward", slice(None)), ("reversed", slice(None, None, -1))):
            out.append(dict(kind="search", name="prior_%s_%d" % (name, count), NR=rings, NS=sectors, MK=260, count=count, Qn=Qn,
                            qmask=qmask, En=c["Dn"][order], emask=c["masks"][order], frame_ids=c["frame_ids"], f=c["f"],
                            min_id=C.MIN_ID, positions=None, max_distance=None, active=1))
    NR, NS = 4, 8
    Dn, masks, clouds = C.places(7, 3, NR, NS, 64)
    En, em = np.stack([Dn[0], Dn[1], Dn[1]]), [masks[0], masks[1], masks[1]]
    pos = np.zeros((31, 3))
    pos[30] = (3.0, 4.0, 0.0)
    base = dict(kind="search", NR=NR, NS=NS, MK=8, count=3, Qn=Dn[1], qmask=masks[1], En=En, emask=em, f=30, min_id=5,
                positions=None, max_distance=None, active=1)
    out.append(dict(base, name="prior_rules_same", frame_ids=np.array([0, 1, 2], dtype=np.int32)))
    out.append(dict(base, name="prior_rules_recent", frame_ids=np.array([25, 26, 27], dtype=np.int32)))
    out.append(dict(base, name="prior_rules_too_recent", frame_ids=np.array([26, 27, 28], dtype=np.int32)))
    out.append(dict(base, name="prior_rules_empty_query", frame_ids=np.array([0, 1, 2], dtype=np.int32),
                    Qn=np.zeros((NR, NS), dtype=F), qmask=0))
    for name, md in (("at", 5.0), ("past", float(np.nextafter(5.0, 6.0)))):
        out.append(dict(base, name="prior_rules_gate_" + name, frame_ids=np.array([0, 1, 2], dtype=np.int32), positions=pos,
                        max_distance=md))
    score = M.search(Dn[0], masks[0], [Dn[1]], [masks[1]], [0], 30, 5, 0.2)["score"]
    for name, thr in (("at", float(score)), ("past", float(np.nextafter(score, F(2))))):
        out.append(dict(base, name="prior_rules_threshold_" + name, count=1, Qn=Dn[0], qmask=masks[0], En=Dn[1][None],
                        emask=[masks[1]], frame_ids=np.array([0], dtype=np.int32), threshold=thr))
    # the slot words of test_insert_stride_overflow_restart_and_idle: MK = 3, stride 2
    for f, count, active in ((0, 0, 1), (1, 1, 1), (2, 1, 1), (3, 2, 1), (4, 2, 1), (6, 3, 1), (6, 3, 0), (6, 0, 1)):
        sc = np.full(3, np.inf, dtype=F)
        sc[:min(count, 1)] = 0.0
        out.append(dict(kind="select", name="prior_slot_f%d_c%d_a%d" % (f, count, active), MK=3, NS=8, scores=sc,
                        shifts=np.zeros(3, dtype=np.int32), frame_ids=np.zeros(3, dtype=np.int32), count=count, active=active,
                        f=f, stride=2, threshold=THRESHOLD))
    return out


def prior_accept():
    """(config, rows): verify=None with a short log; the revisit and the offset scenes with the recorded pairs and costs."""
    row = lambda **kw: dict(dict(name="prior", found=1, status=0, pairs=0, cost=0.0, nlog=0, want=None), **kw)
    return [("prior_no_status", dict(n=64, min_fitness=0.0, max_mean_cost=0.0, ML=256, status=False), [row(), row(found=0)]),
            ("prior_revisit", dict(n=1024, min_fitness=0.3, max_mean_cost=0.25, ML=256, status=True),
             [row(pairs=1000, cost=33.0), row(pairs=1000, cost=28.0, nlog=1), row(found=0)]),
            ("prior_offset", dict(n=1024, min_fitness=0.9, max_mean_cost=0.06, ML=256, status=True),
             [row(pairs=772, cost=77.03), row(pairs=1012, cost=1012 * 0.0269)])]
