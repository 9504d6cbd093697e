"""A second implementation of the loop detector's stages, written the way the kernels work (a 64-lane butterfly for the
shift, a 256-thread strided scan and a tree for select, one thread per stream for accept, strided copies for fetch and insert),
with planted faults.  Without a fault it must equal tests/loop_closure_model.py on every case; with each fault at least one
case must differ (tests/test_loop_closure_edges_cpu.py).  ``answer_model`` and ``answer_second`` give both answers of a case
of tests/loop_closure_edge_cases.py in one comparable form."""
import numpy as np

import loop_closure_edge_cases as EC
import loop_closure_model as M

F = np.float32
LANES, THREADS, WAVES, COPY_STEP = 64, 256, 4, 8 * 256
U64 = (1 << 64) - 1

FAULTS = {
    1: "<= for < at the threshold",
    2: "< for <= in fe + min_id <= f",
    3: "<= at the distance gate",
    4: "a tie goes to the higher entry",
    5: "a tie goes to the higher shift",
    6: "a NaN score wins",
    7: "NS == 64 rotated with a 63-bit mask",
    8: "the rotation turned the other way",
    9: "> for >= at min_fitness",
    10: "< for <= at max_mean_cost",
    11: "one status bit ignored",
    12: "a log write at nlog == ML",
    13: "count left unchanged by insert",
    14: "an untransposed insert",
    15: "a fetch that ignores found",
    16: "a slot granted at count == MK",
    17: "f % stride taken on |f|",
    18: "restart applied to an idle stream",
}


def rotate(m, NS, s, fault=None):
    full = (1 << (63 if fault == 7 and NS == 64 else NS)) - 1
    if s == 0:
        return m & full
    if fault == 8:
        return ((m << s) | (m >> (NS - s))) & full & U64
    return ((m >> s) | ((m << (NS - s)) & U64)) & full


def score_entry(Qn, qmask, E, emask, fault=None):
    """One wave: lane = shift, the query doubled along the sectors, one accumulator per lane, then the butterfly."""
    NR, NS = Qn.shape
    Q2 = np.concatenate([Qn, Qn], axis=1)
    lane = np.arange(LANES)
    sh = np.where(lane < NS, lane, 0)
    acc = np.zeros(LANES, dtype=F)
    for j in range(NS):
        for r in range(NR):
            acc = acc + Q2[r, sh + j] * E[r, j]
    v = np.array([bin(rotate(qmask, NS, int(s), fault) & emask).count("1") for s in sh], dtype=F)
    with np.errstate(all="ignore"):
        d = np.where((lane < NS) & (v > 0), F(1) - acc / v, F(np.inf)).astype(F)
    best = lane.copy()
    off = 32
    while off >= 1:
        od, ob = d[lane ^ off], best[lane ^ off]
        tie = (ob > best) if fault == 5 else (ob < best)
        take = (od < d) | ((od == d) & tie)
        d, best = np.where(take, od, d), np.where(take, ob, best)
        off >>= 1
    return d[0], int(best[0])


def score(c, fault=None):
    """The score kernel on one stream of a search case -> (scores (MK,), shifts (MK,)); entries no wave writes keep NaN / -7."""
    MK, count, f = c["MK"], c["count"], c["f"]
    scores, shifts = np.full(MK, np.nan, dtype=F), np.full(MK, -7, dtype=np.int64)
    blocks = -(-MK // WAVES)
    for e in range(blocks * WAVES):
        if e >= MK:
            continue
        ok = c["active"] != 0 and e < count
        fe = 0
        if ok:
            fe = int(c["frame_ids"][e])
            ok = fe + c["min_id"] < f if fault == 2 else fe + c["min_id"] <= f
        if ok and c["positions"] is not None and c["max_distance"] is not None:
            p = c["positions"]
            ok = 0 <= f < len(p) and 0 <= fe < len(p)
            if ok:
                dx, dy, dz = p[fe] - p[f]
                d2 = (dx * dx + dy * dy) + dz * dz
                m2 = c["max_distance"] * c["max_distance"]
                ok = bool(d2 <= m2) if fault == 3 else bool(d2 < m2)
        if not ok:
            scores[e], shifts[e] = np.inf, 0
            continue
        scores[e], shifts[e] = score_entry(c["Qn"], c["qmask"], c["En"][e], c["emask"][e] & U64, fault)
    return scores, shifts


def select(c, fault=None):
    """One workgroup: each thread scans its stride ascending, then the tree -> the model's dict."""
    MK, thr = c["MK"], F(c["threshold"])
    act = c["active"] != 0
    red_d, red_e = np.full(THREADS, np.inf, dtype=F), np.full(THREADS, MK, dtype=np.int64)
    if act:
        sc = np.asarray(c["scores"], dtype=F)
        for tid in range(min(THREADS, MK)):
            d, e = F(np.inf), MK
            for i in range(tid, MK, THREADS):
                v = sc[i]
                if fault == 6:
                    take = not (v >= d)
                elif fault == 4:
                    take = v <= d and v < F(np.inf)
                else:
                    take = v < d
                if take:
                    d, e = v, i
            red_d[tid], red_e[tid] = d, e
    half = THREADS // 2
    while half >= 1:
        for tid in range(half):
            od, oe = red_d[tid + half], red_e[tid + half]
            tie = oe > red_e[tid] if fault == 4 else oe < red_e[tid]
            if fault == 4 and oe == MK:
                tie = False
            lower = (not (od >= red_d[tid])) and oe < MK if fault == 6 else od < red_d[tid]
            if lower or (od == red_d[tid] and tie):
                red_d[tid], red_e[tid] = od, oe
        half >>= 1
    d, e = red_d[0], int(red_e[0])
    any_ = e < MK
    hit = any_ and (d <= thr if fault == 1 else d < thr)
    out = dict(match=(int(hit), e if any_ else -1, int(c["frame_ids"][e]) if any_ else -1, int(c["shifts"][e]) if any_ else 0),
               score=d, found=int(hit), slot=-1, overflow=False, row=int(c["shifts"][e]) if hit else None)
    if act:
        f, cnt, stride = c["f"], c["count"], c["stride"]
        on = abs(f) % stride == 0 if fault == 17 else (f >= 0 and f % stride == 0)
        if on:
            if cnt < MK or (fault == 16 and cnt == MK):
                out["slot"] = int(cnt)
            else:
                out["overflow"] = True
    return out


def accept(cfg, st, fault=None):
    """One thread per stream of ``EC.accept_streams`` -> the model's dicts."""
    S, outs = len(st["found"]), []
    refuse = M.FEW_PAIRS if fault == 11 else M.FEW_PAIRS | M.BAD_PIVOT
    for s in range(S):
        out = dict(accepted=0, nlog=int(st["nlog"][s]), overflow=False, record=None)
        outs.append(out)
        if st["found"][s] == 0:
            continue
        pairs, cost = 0, np.float64(0.0)
        if cfg["status"]:
            pairs, cost = int(st["pairs"][s]), np.float64(st["cost"][s])
            if st["status"][s] & refuse:
                continue
            need = np.float64(cfg["min_fitness"]) * np.float64(cfg["n"])
            if not (np.float64(pairs) > need if fault == 9 else np.float64(pairs) >= need):
                continue
            with np.errstate(all="ignore"):
                mean = cost / np.float64(pairs)
            bound = np.float64(cfg["max_mean_cost"])
            if not (mean < bound if fault == 10 else mean <= bound):
                continue
        l = int(st["nlog"][s])
        if (l > cfg["ML"]) if fault == 12 else (l >= cfg["ML"]):
            out["overflow"] = True
            continue
        m = st["match"][s]
        out.update(accepted=1, nlog=l + 1, record=(np.array([m[2], st["f"][s], m[3], pairs], dtype=np.int32), st["T"][s].copy(),
                                                   np.array([np.float64(st["score"][s]), cost])))
    return outs


def accept_model(cfg, st):
    return [M.accept(int(st["found"][s]), tuple(st["match"][s]), st["score"][s], int(st["f"][s]), st["T"][s],
                     int(st["status"][s]) if cfg["status"] else None, st["pairs"][s], st["cost"][s], cfg["n"],
                     cfg["min_fitness"], cfg["max_mean_cost"], int(st["nlog"][s]), cfg["ML"]) for s in range(len(st["found"]))]


def same_accept(a, b):
    for x, y in zip(a, b):
        if (x["accepted"], x["nlog"], x["overflow"], x["record"] is None) != (y["accepted"], y["nlog"], y["overflow"],
                                                                               y["record"] is None):
            return False
        if x["record"] is not None and any(p.tobytes() != q.tobytes() for p, q in zip(x["record"], y["record"])):
            return False
    return True


def insert(slot, f, Qn, qmask, cloud, MK, count, fault=None):
    """The strided copies of one stream -> (None or the model's dict, the count word afterwards)."""
    if slot < 0 or slot >= MK:
        return None, count
    NR, NS = Qn.shape
    cells, flat = NR * NS, np.asarray(Qn, dtype=F).reshape(-1)
    E = np.zeros(cells, dtype=F)
    for first in range(COPY_STEP):
        for i in range(first, cells, COPY_STEP):
            j, r = divmod(i, NR)
            E[i] = flat[i] if fault == 14 else flat[r * NS + j]
    kept = None
    if cloud is not None:
        src, kept = np.asarray(cloud, dtype=F).reshape(-1), np.zeros(cloud.size, dtype=F)
        for i in range(0, cloud.size, COPY_STEP):
            kept[i:i + COPY_STEP] = src[i:i + COPY_STEP]
        kept = kept.reshape(cloud.shape)
    new = count if fault == 13 else slot + 1
    return dict(entry=int(slot), desc=E.reshape(NS, NR), mask=int(qmask), frame=int(f), cloud=kept, count=new), new


def fetch(found, match, db_cloud, MK, fault=None):
    e = match[1]
    if (found == 0 and fault != 15) or e < 0 or e >= MK:
        return None
    return np.asarray(db_cloud, dtype=F)[e].copy()


def build_words(active, restart, count, nlog, epoch, fault=None):
    if active == 0 and fault != 18:
        return count, nlog, epoch
    if restart != 0:
        return 0, 0, epoch + 1
    return count, nlog, epoch


# ---- both answers of a case, comparable ----------------------------------------------------------------------------------------

def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32).tolist()


def _select_key(o):
    return (tuple(o["match"]), _bits([o["score"]])[0], o["found"], o["slot"], o["overflow"], o["row"])


def model_scores(c):
    """(scores (MK,), shifts (MK,)) as the score kernel must leave them; entries at or past the count hold +inf and 0."""
    MK, count = c["MK"], c["count"]
    scores, shifts = np.full(MK, np.inf, dtype=F), np.zeros(MK, dtype=np.int64)
    if c["active"] and count:
        out = M.search(c["Qn"], c["qmask"], c["En"], [m & U64 for m in c["emask"]], c["frame_ids"], c["f"], c["min_id"],
                       c.get("threshold", EC.THRESHOLD), c["positions"], c["max_distance"])
        scores[:count], shifts[:count] = out["scores"], out["shifts"]
    return scores, shifts


def _as_select(c, scores, shifts):
    ids = np.zeros(c["MK"], dtype=np.int64)
    ids[:c["count"]] = c["frame_ids"]
    return dict(MK=c["MK"], scores=scores, shifts=shifts, frame_ids=ids, count=c["count"], active=c["active"], f=c["f"], stride=1,
                threshold=c.get("threshold", EC.THRESHOLD))


def answer_model(c):
    if c["kind"] == "search":
        scores, shifts = model_scores(c)
        s = _as_select(c, scores, shifts)
        o = M.select(s["scores"], s["shifts"], s["frame_ids"], s["count"], s["active"], s["f"], s["stride"], s["threshold"], s["MK"])
        return (_bits(scores), shifts.tolist(), _select_key(o))
    o = M.select(c["scores"], c["shifts"], c["frame_ids"], c["count"], c["active"], c["f"], c["stride"], c["threshold"], c["MK"])
    return _select_key(o)


SCORE_FAULTS = (2, 3, 5, 7, 8)                           # the faults that live in the score kernel
_scored = {}


def answer_second(c, fault=None):
    if c["kind"] == "search":
        key = (c["name"], fault if fault in SCORE_FAULTS else None)
        if key not in _scored:
            _scored[key] = score(c, key[1])
        scores, shifts = _scored[key]
        return (_bits(scores), shifts.tolist(), _select_key(select(_as_select(c, scores, shifts), fault)))
    return _select_key(select(c, fault))
