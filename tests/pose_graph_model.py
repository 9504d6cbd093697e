"""Float64 NumPy model of the pose-graph backend, in the kernels' source order.

What csrc/pose_graph.hip computes, written operation by operation in the same order wherever the device result has to agree
to the bit (products of transforms, the quaternion, the retraction, ``Omega e``, the chi2 term, the sums of ``block_sum``,
the gain ratio and the lambda schedule).  The solve is offered three ways: the kernel's block-Jacobi preconditioned conjugate
gradients with its stopping rule (``solver="cg"``), ``numpy.linalg.solve`` on the dense system (``"dense"``) and
``scipy.sparse.linalg.spsolve`` (``"sparse"``).  ``faults`` plants one of the mistakes the tables must catch.
"""
import numpy as np

THREADS = 256                                    # csrc/pose_graph.hpp: PG_THREADS
SLOT = 136
E_, OE, HII, HIJ, HJJ, BI, BJ, CHI = 0, 6, 12, 48, 84, 120, 126, 132
CONVERGED, TRIVIAL, NONFINITE = 1, 2, 4
OM_ODOMETRY = np.diag([2.0, 2, 2, 5, 5, 5])
OM_LOOP_FAR = np.diag([.1, .1, .1, .5, .5, .5])
OM_ABSOLUTE = np.diag([1.0, 1, 1, .001, .001, .001])
FAULTS = ("no_sign_rule", "z_for_zinv", "loop_rule_5", "fixed_row_in", "reject_keeps_trial")


def default_information(kind, i=0, j=0, faults=()):
    if kind == "absolute":
        return OM_ABSOLUTE.copy()
    if kind == "odometry" or abs(int(i) - int(j)) <= (5 if "loop_rule_5" in faults else 4):
        return OM_ODOMETRY.copy()
    return OM_LOOP_FAR.copy()


# ---- SE(3), in source order ----------------------------------------------------------------------------------------------

def mul(a, b):
    """a . b for (..., 4, 4): se3_mul's order, (a0 b0 + a1 b1) + a2 b2, then + a3 in the last column."""
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    c = np.zeros(a.shape)
    c[..., 3, 3] = 1.0
    for i in range(3):
        for j in range(4):
            s = (a[..., i, 0] * b[..., 0, j] + a[..., i, 1] * b[..., 1, j]) + a[..., i, 2] * b[..., 2, j]
            if j == 3:
                s = s + a[..., i, 3]
            c[..., i, j] = s
    return c


def rigid_inv(a):
    a = np.asarray(a, np.float64)
    r = np.zeros(a.shape)
    r[..., 3, 3] = 1.0
    for i in range(3):
        for j in range(3):
            r[..., i, j] = a[..., j, i]
        r[..., i, 3] = -((a[..., 0, i] * a[..., 0, 3] + a[..., 1, i] * a[..., 1, 3]) + a[..., 2, i] * a[..., 2, 3])
    return r


def quat(a):
    """(..., 4) [w x y z]: Shepperd's branch selection, normalised, no sign rule.  Also returns the branch taken."""
    a = np.asarray(a, np.float64)
    r00, r01, r02 = a[..., 0, 0], a[..., 0, 1], a[..., 0, 2]
    r10, r11, r12 = a[..., 1, 0], a[..., 1, 1], a[..., 1, 2]
    r20, r21, r22 = a[..., 2, 0], a[..., 2, 1], a[..., 2, 2]
    tr = (r00 + r11) + r22
    b0 = (tr >= r00) & (tr >= r11) & (tr >= r22)
    b1 = ~b0 & (r00 >= r11) & (r00 >= r22)
    b2 = ~b0 & ~b1 & (r11 >= r22)
    branch = np.where(b0, 0, np.where(b1, 1, np.where(b2, 2, 3)))
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.sqrt(1.0 + tr); k = 0.5 / u
        q0 = np.stack([0.5 * u, (r21 - r12) * k, (r02 - r20) * k, (r10 - r01) * k], -1)
        u = np.sqrt(((1.0 + r00) - r11) - r22); k = 0.5 / u
        q1 = np.stack([(r21 - r12) * k, 0.5 * u, (r01 + r10) * k, (r02 + r20) * k], -1)
        u = np.sqrt(((1.0 - r00) + r11) - r22); k = 0.5 / u
        q2 = np.stack([(r02 - r20) * k, (r01 + r10) * k, 0.5 * u, (r12 + r21) * k], -1)
        u = np.sqrt(((1.0 - r00) - r11) + r22); k = 0.5 / u
        q3 = np.stack([(r10 - r01) * k, (r02 + r20) * k, (r12 + r21) * k, 0.5 * u], -1)
    br = branch[..., None]
    q = np.where(br == 0, q0, np.where(br == 1, q1, np.where(br == 2, q2, q3)))
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    inv = 1.0 / np.sqrt(((w * w + x * x) + y * y) + z * z)
    return q * inv[..., None], branch


def set_rotation(a, q):
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    a[..., 0, 0] = 1.0 - 2.0 * (yy + zz); a[..., 0, 1] = 2.0 * (xy - wz); a[..., 0, 2] = 2.0 * (xz + wy)
    a[..., 1, 0] = 2.0 * (xy + wz); a[..., 1, 1] = 1.0 - 2.0 * (xx + zz); a[..., 1, 2] = 2.0 * (yz - wx)
    a[..., 2, 0] = 2.0 * (xz - wy); a[..., 2, 1] = 2.0 * (yz + wx); a[..., 2, 2] = 1.0 - 2.0 * (xx + yy)
    return a


def retract(x, d):
    """x (..., 4, 4), d (..., 6) -> x . D(d), the rotation rebuilt from its normalised quaternion."""
    x, d = np.asarray(x, np.float64), np.asarray(d, np.float64)
    n2 = (d[..., 3] * d[..., 3] + d[..., 4] * d[..., 4]) + d[..., 5] * d[..., 5]
    big = n2 > 1.0
    with np.errstate(invalid="ignore", divide="ignore"):
        inv = 1.0 / np.sqrt(n2)
        w = np.where(big, 0.0, np.sqrt(1.0 - n2))
        v = np.where(big[..., None], d[..., 3:] * inv[..., None], d[..., 3:])
    D = np.zeros(x.shape)
    D[..., 3, 3] = 1.0
    set_rotation(D, np.concatenate([w[..., None], v], -1))
    D[..., :3, 3] = d[..., :3]
    t = mul(x, D)
    return set_rotation(t, quat(t)[0])


def pose(axis, angle, t=(0, 0, 0)):
    """A rigid transform from an axis, an angle in radians and a translation (Rodrigues; not mirrored by any kernel)."""
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    T[:3, 3] = t
    return T


# ---- the graph ------------------------------------------------------------------------------------------------------------

class Graph:
    """One stream.  X (n, 4, 4) vertices, Z (n, 4, 4) chain measurements (Z[k]: pair (k-1, k); Z[0] unused); loops: (i, j, Z,
    Omega); absolutes: (i, G, Omega).  N, ML, MA: the device capacities, which place the edge ids."""

    def __init__(self, N, ML=8, MA=8, fix_first=True):
        self.N, self.ML, self.MA, self.fix_first = int(N), int(ML), int(MA), bool(fix_first)
        self.X = np.eye(4)[None].copy()
        self.Z = np.eye(4)[None].copy()
        self.loops, self.absolutes = [], []

    @property
    def n(self):
        return len(self.X)

    @property
    def E(self):
        return self.N + self.ML + self.MA

    def append(self, Z):
        Z = np.asarray(Z, np.float64)
        self.X = np.concatenate([self.X, mul(self.X[-1], Z)[None]])
        self.Z = np.concatenate([self.Z, Z[None]])

    def add_loop(self, i, j, Z, Om=None, faults=()):
        self.loops.append((int(i), int(j), np.asarray(Z, np.float64),
                           default_information("loop", i, j, faults) if Om is None else np.asarray(Om, np.float64)))

    def add_absolute(self, i, G, Om=None):
        self.absolutes.append((int(i), np.asarray(G, np.float64),
                               default_information("absolute") if Om is None else np.asarray(Om, np.float64)))

    def free(self):
        f = np.ones(self.n, bool)
        if self.fix_first:
            f[0] = False
        return f

    def edges(self):
        """ids, vi, vj, Z, Om, absolute: every edge in id order."""
        n = self.n
        ids = list(range(1, n)) + [self.N + l for l in range(len(self.loops))] + \
            [self.N + self.ML + a for a in range(len(self.absolutes))]
        vi = list(range(0, n - 1)) + [l[0] for l in self.loops] + [a[0] for a in self.absolutes]
        vj = list(range(1, n)) + [l[1] for l in self.loops] + [a[0] for a in self.absolutes]
        Z = [self.Z[k] for k in range(1, n)] + [l[2] for l in self.loops] + [a[1] for a in self.absolutes]
        Om = [OM_ODOMETRY] * (n - 1) + [l[3] for l in self.loops] + [a[2] for a in self.absolutes]
        ab = [False] * (n - 1 + len(self.loops)) + [True] * len(self.absolutes)
        return (np.array(ids, int), np.array(vi, int), np.array(vj, int), np.array(Z).reshape(-1, 4, 4),
                np.array(Om).reshape(-1, 6, 6), np.array(ab, bool))

    def incidence(self):
        """Per vertex the entries edge id * 2 + side of its loop and absolute edges, in edge order: what the host writes."""
        inc = [[] for _ in range(self.n)]
        for l, (i, j, _, _) in enumerate(self.loops):
            inc[i].append((self.N + l) * 2)
            inc[j].append((self.N + l) * 2 + 1)
        for a, (i, _, _) in enumerate(self.absolutes):
            inc[i].append((self.N + self.ML + a) * 2 + 1)
        return inc


def skew(t):
    z = np.zeros(t.shape[:-1])
    return np.stack([np.stack([z, -t[..., 2], t[..., 1]], -1), np.stack([t[..., 2], z, -t[..., 0]], -1),
                     np.stack([-t[..., 1], t[..., 0], z], -1)], -2)


def edge_error(Xi, Xj, Z, Om, absolute, faults=()):
    """-> dict(e, Oe, chi, D, A, q, sg): the error of edges given both ends' poses, in the kernel's order."""
    A = np.where(absolute[:, None, None], Xj, mul(rigid_inv(Xi), Xj))
    D = mul(Z if "z_for_zinv" in faults else rigid_inv(Z), A)
    q, branch = quat(D)
    sg = np.where(q[:, 0] < 0.0, -1.0, 1.0)
    e = np.concatenate([D[:, :3, 3], sg[:, None] * q[:, 1:]], -1)
    Oe = np.zeros_like(e)
    for r in range(6):
        t = Om[:, r, 0] * e[:, 0]
        for m in range(1, 6):
            t = t + Om[:, r, m] * e[:, m]
        Oe[:, r] = t
    chi = e[:, 0] * Oe[:, 0]
    for m in range(1, 6):
        chi = chi + e[:, m] * Oe[:, m]
    return dict(e=e, Oe=Oe, chi=chi, D=D, A=A, q=q, sg=sg, branch=branch)


def jacobians(err, Z, absolute, faults=()):
    """-> Ji, Jj (E, 6, 6), analytic (section 25)."""
    D, A, q = err["D"], err["A"], err["q"]
    sg = np.ones_like(err["sg"]) if "no_sign_rule" in faults else err["sg"]
    n = len(D)
    w, v = q[:, 0], q[:, 1:]
    I3 = np.eye(3)[None]
    Jj = np.zeros((n, 6, 6)); Ji = np.zeros((n, 6, 6))
    Jj[:, :3, :3] = D[:, :3, :3]
    Jj[:, 3:, 3:] = sg[:, None, None] * (w[:, None, None] * I3 + skew(v))
    RZt = np.swapaxes(Z[:, :3, :3], 1, 2)
    Ji[:, :3, :3] = -RZt
    Ji[:, :3, 3:] = 2.0 * (RZt @ skew(A[:, :3, 3]))
    Ji[:, 3:, 3:] = sg[:, None, None] * ((-w[:, None, None] * I3 + skew(v)) @ RZt)
    Ji[absolute] = 0.0
    return Ji, Jj


def chi_terms(g, X, faults=()):
    """The chi2 term of every edge at the poses X, placed at its id: (E,) with zeros elsewhere."""
    ids, vi, vj, Z, Om, ab = g.edges()
    out = np.zeros(g.E)
    if len(ids):
        out[ids] = edge_error(X[vi], X[vj], Z, Om, ab, faults)["chi"]
    return out


def linearise(g, X=None, faults=()):
    """-> slots (E, 136) with zeros where there is no edge, and the edge table."""
    X = g.X if X is None else X
    ids, vi, vj, Z, Om, ab = g.edges()
    slots = np.zeros((g.E, SLOT))
    if not len(ids):
        return slots, (ids, vi, vj, ab)
    err = edge_error(X[vi], X[vj], Z, Om, ab, faults)
    Ji, Jj = jacobians(err, Z, ab, faults)
    JiT, JjT = np.swapaxes(Ji, 1, 2), np.swapaxes(Jj, 1, 2)
    s = slots[ids]
    s[:, E_:E_ + 6], s[:, OE:OE + 6], s[:, CHI] = err["e"], err["Oe"], err["chi"]
    s[:, HII:HII + 36] = (JiT @ (Om @ Ji)).reshape(-1, 36)
    s[:, HIJ:HIJ + 36] = (JiT @ (Om @ Jj)).reshape(-1, 36)
    s[:, HJJ:HJJ + 36] = (JjT @ (Om @ Jj)).reshape(-1, 36)
    s[:, BI:BI + 6] = (JiT @ err["Oe"][:, :, None])[:, :, 0]
    s[:, BJ:BJ + 6] = (JjT @ err["Oe"][:, :, None])[:, :, 0]
    slots[ids] = s
    return slots, (ids, vi, vj, ab)


def block_sum(values):
    """The kernels' fixed-order sum of values[0], values[1], ...: thread t adds its elements t, t + 256, ... in order; the 64
    lanes of a wave are halved (32, .., 1), then the four wave results (2, 1)."""
    v = np.asarray(values, np.float64)
    pad = (-len(v)) % THREADS
    rows = np.concatenate([v, np.zeros(pad)]).reshape(-1, THREADS)
    acc = np.zeros(THREADS)
    for row in rows:
        acc = acc + row
    w = acc.reshape(THREADS // 64, 64).copy()
    off = 32
    while off >= 1:
        w[:, :off] = w[:, :off] + w[:, off:2 * off]
        off //= 2
    t = w[:, 0].copy()
    off = THREADS // 128
    while off >= 1:
        t[:off] = t[:off] + t[off:2 * off]
        off //= 2
    return float(t[0])


def gather_b(g, slots, faults=()):
    """b (n, 6) per vertex in the kernels' order: chain edge v, chain edge v + 1, the incidence list; zero at a fixed vertex."""
    n = g.n
    inc = g.incidence()
    b = np.zeros((n, 6))
    for v in range(n):
        if v >= 1:
            b[v] = b[v] + slots[v, BJ:BJ + 6]
        if v + 1 < n:
            b[v] = b[v] + slots[v + 1, BI:BI + 6]
        for ent in inc[v]:
            o = BJ if ent & 1 else BI
            b[v] = b[v] + slots[ent >> 1, o:o + 6]
    if "fixed_row_in" not in faults:
        b[~g.free()] = 0.0
    return b


def assemble(g, slots, table, faults=()):
    """Dense H (6n, 6n) and b (6n,) over every vertex; the rows and columns of fixed vertices are zero."""
    ids, vi, vj, ab = table
    n = g.n
    H = np.zeros((6 * n, 6 * n))
    for k, id_ in enumerate(ids):
        i, j = vi[k], vj[k]
        sl = slots[id_]
        H[6 * j:6 * j + 6, 6 * j:6 * j + 6] += sl[HJJ:HJJ + 36].reshape(6, 6)
        if not ab[k]:
            H[6 * i:6 * i + 6, 6 * i:6 * i + 6] += sl[HII:HII + 36].reshape(6, 6)
            H[6 * i:6 * i + 6, 6 * j:6 * j + 6] += sl[HIJ:HIJ + 36].reshape(6, 6)
            H[6 * j:6 * j + 6, 6 * i:6 * i + 6] += sl[HIJ:HIJ + 36].reshape(6, 6).T
    b = gather_b(g, slots, faults).reshape(-1)
    if "fixed_row_in" not in faults:
        keep = np.repeat(g.free(), 6)
        H[~keep] = 0.0
        H[:, ~keep] = 0.0
    return H, b


def free_index(g, faults=()):
    f = np.ones(g.n, bool) if "fixed_row_in" in faults else g.free()
    return np.flatnonzero(np.repeat(f, 6))


def pcg(A, b, M_blocks, tol, iters):
    """Block-Jacobi preconditioned CG on A x = -b from x = 0 with the kernel's stopping rule -> x, used, |r| / |b|."""
    def prec(r):
        return np.einsum("vij,vj->vi", M_blocks, r.reshape(-1, 6)).reshape(-1)
    x = np.zeros_like(b)
    r = -b
    z = prec(r)
    p = z.copy()
    rz = r @ z
    bnorm = np.sqrt(b @ b)
    rr, used = bnorm * bnorm, 0
    for k in range(iters):
        Ap = A @ p
        pAp = p @ Ap
        if not pAp > 0.0:
            break
        alpha = rz / pAp
        x = x + alpha * p
        r = r - alpha * Ap
        z = prec(r)
        rz_n, rr = r @ z, r @ r
        used = k + 1
        if np.sqrt(rr) <= tol * bnorm:
            break
        p = z + (rz_n / rz) * p
        rz = rz_n
    return x, used, np.sqrt(rr) / bnorm


def solve(g, H, b, lam, solver="dense", pcg_tol=1e-8, pcg_iters=None, faults=()):
    """delta (n, 6) of (H + lam I) delta = -b over the free vertices -> delta, (used, relres)."""
    idx = free_index(g, faults)
    A = H[np.ix_(idx, idx)] + lam * np.eye(len(idx))
    rhs = b[idx]
    info = (0, 0.0)
    if solver == "dense":
        x = np.linalg.solve(A, -rhs)
    elif solver == "sparse":
        import scipy.sparse
        import scipy.sparse.linalg
        x = scipy.sparse.linalg.spsolve(scipy.sparse.csc_matrix(A), -rhs)
    else:
        blocks = np.stack([np.linalg.inv(A[k:k + 6, k:k + 6]) for k in range(0, len(idx), 6)])
        x, used, rel = pcg(A, rhs, blocks, pcg_tol, 12 * g.N if pcg_iters is None else pcg_iters)
        info = (used, rel)
    d = np.zeros(6 * g.n)
    d[idx] = x
    return d.reshape(-1, 6), info


def scaled_condition(g, H, lam, faults=()):
    """Condition number of the Jacobi-scaled (diagonal-scaled) H + lam I over the free vertices."""
    idx = free_index(g, faults)
    A = H[np.ix_(idx, idx)] + lam * np.eye(len(idx))
    s = 1.0 / np.sqrt(np.diag(A))
    return np.linalg.cond(A * s[:, None] * s[None, :])


def judge(g, X, delta, b, lam, nu, chi, faults=()):
    """One accept / reject decision in the judge kernel's order.  b (n, 6) gathered.  -> dict(X, lam, nu, chi, status,
    accepted, chi_new, rho, Xt)."""
    free = np.ones(g.n, bool) if "fixed_row_in" in faults else g.free()
    Xt = X.copy()
    Xt[free] = retract(X[free], delta[free])
    chi_n = block_sum(chi_terms(g, Xt, faults))
    terms = np.zeros(g.n)
    for v in np.flatnonzero(free):
        d = delta[v]
        t = d[0] * (lam * d[0] - b[v, 0])
        for m in range(1, 6):
            t = t + d[m] * (lam * d[m] - b[v, m])
        terms[v] = t
    scale = block_sum(terms)
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = (chi - chi_n) / scale
    ok = bool(rho > 0.0 and np.isfinite(chi_n))
    status = 0
    if ok:
        t = 2.0 * rho - 1.0
        a = 1.0 - (t * t) * t
        lam, nu = lam * max(1.0 / 3.0, a), 2.0
        if chi - chi_n <= 1e-9 * chi:
            status = CONVERGED
        chi, X = chi_n, Xt
    else:
        lam, nu = lam * nu, 2.0 * nu
        if "reject_keeps_trial" in faults:
            X = Xt
    return dict(X=X, lam=lam, nu=nu, chi=chi, status=status, accepted=ok, chi_new=chi_n, rho=rho, Xt=Xt)


def optimize(g, iters=20, solver="dense", pcg_tol=1e-8, pcg_iters=None, faults=()):
    """Levenberg-Marquardt on the graph, in place (g.X).  -> dict(status, chi2, chi2_0, lam, steps)."""
    if g.n <= 1 or (not g.loops and not g.absolutes):
        return dict(status=CONVERGED | TRIVIAL, chi2=0.0, chi2_0=0.0, lam=None, steps=[])
    lam = nu = None
    status, steps, chi0, chi = 0, [], None, None
    for it in range(iters):
        slots, table = linearise(g, g.X, faults)
        chi = block_sum(slots[:, CHI])
        chi0 = chi if chi0 is None else chi0
        if not np.isfinite(chi):
            status = NONFINITE
            break
        H, b = assemble(g, slots, table, faults)
        if it == 0:
            lam, nu = 1e-5 * np.max(np.diag(H)[free_index(g, faults)]), 2.0
        if np.max(np.abs(b)) <= 1e-12:
            status = CONVERGED
            break
        delta, info = solve(g, H, b, lam, solver, pcg_tol, pcg_iters, faults)
        out = judge(g, g.X, delta, b.reshape(-1, 6), lam, nu, chi, faults)
        steps.append(dict(lam=lam, chi=chi, chi_new=out["chi_new"], rho=out["rho"], accepted=out["accepted"], pcg=info))
        g.X, lam, nu, chi = out["X"], out["lam"], out["nu"], out["chi"]
        if out["status"]:
            status = out["status"]
            break
    return dict(status=status, chi2=chi, chi2_0=chi0, lam=lam, steps=steps)


def distance(Xa, Xb):
    """(max translation distance, max rotation angle in radians) between two pose arrays."""
    d = rigid_inv(Xa) @ Xb
    c = np.clip((np.trace(d[:, :3, :3], axis1=1, axis2=2) - 1.0) / 2.0, -1.0, 1.0)
    s = 0.5 * np.linalg.norm(np.stack([d[:, 2, 1] - d[:, 1, 2], d[:, 0, 2] - d[:, 2, 0], d[:, 1, 0] - d[:, 0, 1]], -1), axis=-1)
    return float(np.max(np.linalg.norm(Xa[:, :3, 3] - Xb[:, :3, 3], axis=-1))), float(np.max(np.arctan2(s, c)))
