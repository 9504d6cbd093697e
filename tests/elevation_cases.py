"""Inputs of the translation-search tests, shared by the CPU and the GPU files: lattice clouds whose
offset is known in whole cells, the edge rows of the grid arithmetic, the table of search-rule cases with a second,
independently written implementation that can be told to make one mistake (``variant(..., fault=...)``), and the whole-chain
scene whose return passes 2 m beside the start."""
import numpy as np

import elevation_model as EM
import loop_closure_cases as C
import loop_closure_model as LM

F = np.float32
Z_OFFSET = 2.0
SECTORS = 60
SMALL = dict(cells=16, cell_size=1.0, window=3, yaw_div=2, yaw_half=1, z_step=0.25, tolerance=4, min_agreement=0.5)
up_, down_ = lambda v: np.nextafter(F(v), F(np.inf)), lambda v: np.nextafter(F(v), F(-np.inf))


def lattice(seed, p, fill=0.3, margin=None, levels=(1, 40)):
    """(m, 3) fp64: one point at the centre of a random ``fill`` of the cells that lie ``margin`` (default: the window) inside
    the grid, each at the middle of a random level, so that a move by whole cells changes no decision."""
    rng = np.random.default_rng(seed)
    G, c, zs = p["cells"], p["cell_size"], p["z_step"]
    m = p["window"] if margin is None else margin
    on = rng.random((G, G)) < fill
    on[:m], on[G - m:], on[:, :m], on[:, G - m:] = False, False, False, False
    i, j = np.nonzero(on)
    lev = rng.integers(levels[0], levels[1], len(i))
    return np.stack([(i - G // 2 + 0.5) * c, (j - G // 2 + 0.5) * c, (lev + 0.5) * zs - Z_OFFSET], axis=1)


def seen_from(cloud, shift, k, a, b, p, sectors=SECTORS):
    """The stored cloud as the query's sensor sees it when the query's pose in the stored frame is [Rz(theta_k), (a c, b c, 0)]:
    p_query = R^T (p_stored - t)."""
    t = EM.angle(shift, k, sectors, p["yaw_div"], p["yaw_half"])
    R = np.array([[np.cos(t), -np.sin(t), 0.0], [np.sin(t), np.cos(t), 0.0], [0.0, 0.0, 1.0]])
    return (np.asarray(cloud, dtype=np.float64) - np.array([a * p["cell_size"], b * p["cell_size"], 0.0])) @ R


def edge_rows(p, z_offset=Z_OFFSET):
    """(m, 3) fp32 rows on every edge of the grid arithmetic at the identity rotation (xr = x exactly): x / c on an integer
    and on its two fp32 neighbours, the grid's outer edges, h at 0 and beside it, the levels 254 / 255, an infinite h / zs,
    and NaN / +-Inf in every column.  Rows of one group lie in different columns of the other axis."""
    G, c, zs = p["cells"], F(p["cell_size"]), F(p["z_step"])
    rows = []
    lane = lambda r: (F(r % (G - 2)) - F(G // 2) + F(1.5)) * c
    for axis in (0, 1):
        for k in (-G // 2, -1, 0, 1, G // 2 - 1, G // 2):
            v = F(k) * c
            for r, e in enumerate((down_(down_(v)), down_(v), v, up_(v), up_(up_(v)))):
                row = [lane(r + 3 * axis + k), lane(r + 3 * axis + k), F(0.3) + F(r) * zs]
                row[axis] = e
                rows.append(tuple(row))
    z0 = F(-z_offset)
    for r, z in enumerate((z0, up_(z0), down_(z0), z0 + np.nextafter(F(0), F(1)))):          # h = 0 and beside it
        rows.append((F(-2.5) * c, lane(r), z))
    for r, l in enumerate((252.0, 253.0, 254.0, 255.0, 1000.0)):                             # the top of the level scale
        h = F(l) * zs
        for rr, hh in enumerate((down_(h), h, up_(h))):
            rows.append((F(1.5) * c, lane(3 * r + rr), hh - F(z_offset)))
    rows.append((F(2.5) * c, lane(0), F(3.0e38)))                                            # h / zs overflows to +Inf
    for col in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            row = [F(0.5) * c, lane(3 * col + 1), F(1.0)]
            row[col] = bad
            rows.append(tuple(row))
    return np.array(rows, dtype=F)


def planted_cells(cells, G, c=1.0, zs=0.25, z_offset=Z_OFFSET):
    """(m, 3) fp32: one point in the middle of every (i, j, q) given, q in 1..254."""
    a = np.asarray(cells, dtype=np.float64).reshape(-1, 3)
    return np.stack([(a[:, 0] - G // 2 + 0.5) * c, (a[:, 1] - G // 2 + 0.5) * c, (a[:, 2] - 0.5) * zs - z_offset], axis=1).astype(F)


def rule_cases():
    """The table of search rules -> list of dict(name, stored, query, shift, p, length): small enough for the slow second
    implementation, each built so that one rule decides its outcome."""
    p, G = dict(SMALL), SMALL["cells"]
    out = []
    add = lambda name, stored, query, shift=0, length=None, **kw: out.append(
        dict(name=name, stored=np.asarray(stored, dtype=F), query=np.asarray(query, dtype=F), shift=shift, length=length,
             p=dict(p, **kw)))
    lat = lattice(1, p)
    add("lattice moved", lat, seen_from(lat, 7, 2, 2, -1, p), shift=7)
    add("lattice moved the other way", lat, seen_from(lat, 52, 0, -3, 3, p), shift=52)
    add("edge rows", edge_rows(p), lat)
    add("edge rows as the query", lat, edge_rows(p), length=len(edge_rows(p)) - 4)
    add("tie", planted_cells([(6, 8, 5), (10, 8, 5)], G), planted_cells([(8, 8, 5)], G), yaw_half=0)
    add("tie over yaw", planted_cells([(8, 8, 5)], G), planted_cells([(8, 8, 5)], G))
    add("empty query", lat, np.full((4, 3), -50.0))
    add("empty stored", np.full((4, 3), -50.0), lat)
    stored4 = [(5, 5, 9), (5, 9, 20), (9, 5, 30), (9, 9, 40)]
    add("acceptance at the bound", planted_cells(stored4, G),                # A = 4 + 4 = 8 = 0.5 * 4 * min(4, 4)
        planted_cells([(5, 5, 9), (5, 9, 20), (9, 5, 60), (9, 9, 70)], G), yaw_half=0)
    add("acceptance one below", planted_cells(stored4, G),                   # A = 4 + 3 = 7
        planted_cells([(5, 5, 9), (5, 9, 21), (9, 5, 60), (9, 9, 70)], G), yaw_half=0)
    add("fewer query cells than stored", planted_cells(stored4, G), planted_cells([(5, 5, 9), (5, 9, 50)], G), yaw_half=0)
    add("window 0", lat, seen_from(lat, 3, 2, 0, 0, dict(p, yaw_div=1)), shift=3, window=0, yaw_div=1)
    add("one yaw", lat, seen_from(lat, 3, 0, 1, 1, dict(p, yaw_half=0)), shift=3, yaw_half=0)
    low = [(0, 3, 1), (15, 12, 2), (4, 0, 1), (11, 15, 1), (7, 7, 6)]          # low cells on the outer rows and columns
    add("cells on the border", planted_cells([(7, 7, 6), (3, 3, 30)], G), planted_cells(low, G), yaw_half=0)
    add("level zero", planted_cells([(7, 7, 1), (9, 9, 3)], G), planted_cells([(7, 7, 1), (9, 9, 3), (3, 3, 1)], G), yaw_half=0)
    return out


FAULTS = ("h_at_zero_kept", "lower_edge_dropped", "sign_of_a", "sign_of_b", "sign_of_theta", "border_not_zero", "tie_reversed",
          "max_in_acceptance", "level_off_by_one", "acceptance_strict")


def variant(case, z_offset=Z_OFFSET, up="z", fault=None):
    """A second implementation of the step, written the way a kernel would be (row by row, a padded image, a running best),
    that makes the mistake ``fault`` names.  Without a fault it must equal ``elevation_model.search`` on every case."""
    p, stored, query, shift = case["p"], case["stored"], case["query"], case["shift"]
    G, W, L, Yh = p["cells"], p["window"], p["tolerance"], p["yaw_half"]
    c, zs, Y, side = F(p["cell_size"]), F(p["z_step"]), 2 * Yh + 1, 2 * W + 1
    rot = EM.tables(SECTORS, p["yaw_div"], Yh, up)[0]

    def image(cloud, cs, sn, length):
        img = np.zeros((G, G), dtype=np.int64)
        x, y, z = LM.permute(cloud, up)
        for r in range(len(x) if length is None else max(0, min(length, len(x)))):
            if not (np.isfinite(x[r]) and np.isfinite(y[r]) and np.isfinite(z[r])):
                continue
            with np.errstate(all="ignore"):
                fx, fy = np.floor((cs * x[r] - sn * y[r]) / c), np.floor((sn * x[r] + cs * y[r]) / c)
                h = z[r] + F(z_offset)
                lev = np.floor(h / zs)
            low = fx > -G // 2 if fault == "lower_edge_dropped" else fx >= -G // 2
            if not (low and fx < G // 2 and fy >= -G // 2 and fy < G // 2):
                continue
            if h < 0 or (h == 0 and fault != "h_at_zero_kept"):
                continue
            q = 255 if lev >= 254 else int(lev) + (0 if fault == "level_off_by_one" else 1)
            i, j = int(fx) + G // 2, int(fy) + G // 2
            img[i, j] = max(img[i, j], q)
        return img

    E = image(stored, F(1), F(0), None)
    pad = np.full((G + 2 * W, G + 2 * W), 1 if fault == "border_not_zero" else 0, dtype=np.int64)
    pad[W:W + G, W:W + G] = E
    Q = [image(query, rot[shift * Y + k, 0], -rot[shift * Y + k, 1] if fault == "sign_of_theta" else rot[shift * Y + k, 1],
               case["length"]) for k in range(Y)]
    A = np.zeros((Y, side, side), dtype=np.int32)
    best, at = -1, 0
    for k in range(Y):
        cells = [(i, j, Q[k][i, j]) for i in range(G) for j in range(G) if Q[k][i, j]]
        for a in range(-W, W + 1):
            for b in range(-W, W + 1):
                aa, bb = (-a if fault == "sign_of_a" else a), (-b if fault == "sign_of_b" else b)
                total = 0
                for i, j, q in cells:
                    e = pad[i + aa + W, j + bb + W]
                    if e:
                        total += max(0, L - abs(int(q) - int(e)))
                A[k, a + W, b + W] = total
                index = (k * side + a + W) * side + b + W
                if total > best or (total == best and fault == "tie_reversed"):
                    best, at = total, index
    k, a, b = at // (side * side), at // side % side - W, at % side - W
    occ_q, occ_e = [int((q > 0).sum()) for q in Q], int((E > 0).sum())
    least = max(occ_q[k], occ_e) if fault == "max_in_acceptance" else min(occ_q[k], occ_e)
    bound = F(p["min_agreement"]) * F(L * least)
    ok = F(best) > bound if fault == "acceptance_strict" else F(best) >= bound
    rec = dict(found=int(best > 0 and ok), k=k, a=a, b=b, A=int(best), occ_q=occ_q[k], occ_e=occ_e)
    T1 = EM.seed(rec, shift, LM.start_pose(shift, SECTORS, up), SECTORS, p, up)
    return dict(E=E.astype(np.uint8), occ_e=occ_e, Q=np.stack(Q).astype(np.uint8), occ_q=np.array(occ_q, dtype=np.int32), A=A,
                record=rec, T1=T1)


def same(x, y):
    """Whether two results of the step agree in every image, count, score, record word and pose entry."""
    return all(np.array_equal(x[k], y[k]) for k in ("E", "Q", "occ_q", "A", "T1")) and x["occ_e"] == y["occ_e"] \
        and x["record"] == y["record"]


# ---- the whole chain: a return that passes 2 m beside the start -----------------------------------------------------------------

OFFSET_N, OFFSET_MIN_ID, OFFSET_FRAMES = C.REVISIT_N, 30, 40
OFFSET_VERIFY = dict(iters=20, sigma=0.5, max_dist=1.0)
OFFSET_ACCEPT = dict(min_fitness=0.9, max_mean_cost=0.06)       # chosen on the model chain: tests/test_elevation_cpu.py
OFFSET_THRESHOLD = 0.2
OFFSET_TRANSLATION = dict(cells=32, cell_size=1.0, window=8, min_agreement=0.4)
OFFSET_MAX_DISTANCE = 8.0               # about window * cell_size, the advice of DESIGN.md section 26 with translation=


def spiral_path(frames=OFFSET_FRAMES, radius=3.0, out=2.0, turns=0.99, yaw_offset=0.3):
    """Poses of a sensor on one turn of a spiral that starts at the origin and ends ``out`` metres outside its start: every
    late frame passes the early ones at about that distance, none closer."""
    poses = []
    for k in range(frames):
        a = 2 * np.pi * turns * k / (frames - 1)
        r = radius + out * (k / (frames - 1)) ** 2
        poses.append(C.pose(r * np.cos(a) - radius, r * np.sin(a), a + np.pi / 2 + (yaw_offset if k > frames // 2 else 0.0)))
    return poses


def offset_revisit():
    """-> dict(path, frames (K, 1, n, 3) fp32, chain (K, 4, 4), positions (K, 3)) as ``loop_closure_cases.revisit`` lays them
    out, one stream, in the same room."""
    if not _OFFSET:
        pts = C.world_points(C.scene(3, half=10.0, half_y=6.0, centre=(2.0, 1.5)), 20000, 4)
        path = spiral_path()
        frames = [C.scan(pts, T, OFFSET_N, 100 + k) for k, T in enumerate(path)]
        rng = np.random.default_rng(5)
        chain, X = [np.eye(4)], [np.eye(4)]
        for k in range(1, len(path)):
            drift = np.eye(4)
            ang = rng.normal() * 0.004
            drift[:2, :2] = [[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]]
            drift[:3, 3] = rng.normal(size=3) * 0.02
            chain.append((np.linalg.inv(path[k - 1]) @ path[k]) @ drift)
            X.append(X[-1] @ chain[-1])
        _OFFSET.update(path=path, frames=np.stack(frames)[:, None], chain=np.stack(chain), positions=np.stack(X)[:, :3, 3])
    return _OFFSET


_OFFSET = {}
