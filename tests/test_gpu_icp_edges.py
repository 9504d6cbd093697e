"""Every op of the knn refiner (csrc/icp.hip) at its smallest shapes and on every edge of its contract, against the NumPy
fp64 model (tests/icp_model.py) on the cases of tests/icp_cases.py, which tests/test_icp_cases_cpu.py proves to hold what
their names say.  No whole registration, no captured graph: one launch per check.

Guard bands.  Every tensor an op writes is a view into a larger allocation with 256 bytes of 0xA5 on either side, checked
after the call; every pure output is pre-filled with a NaN (or an integer) of a fixed bit pattern, so "written" and "left
alone" are told apart to the bit.

Bounds (those of tests/test_gpu_icp.py).  Normals: 1 - |n . n_model| <= 64 eps64 / gap, length within 2^-23 of 1,
eigenvalues within 64 eps64 of the largest.  Queries: 1 ulp of fp32, exact for identity poses.  Sums: 1e-12 of the sum of
the terms' magnitudes per term, per workgroup row; the pair count exact; two runs the same bits.  Steps and poses: 1e-10,
norm-wise relative; sum, cost, pairs and status exact.  Maps: every array bit for bit."""
import copy

import numpy as np
import pytest
import torch

import icp_cases as cases
import icp_model as model
from pwclonet_pylidarslam_amd import _lib, registration

pytestmark = pytest.mark.gpu

F32, F64, I32 = torch.float32, torch.float64, torch.int32
FILL = {F64: (torch.int64, 0x7FF8DEAD0000BEEF), F32: (torch.int32, 0x7FC0BEEF), I32: (torch.int32, cases.SENTINEL_I32),
        torch.uint8: (torch.uint8, 0x3C)}
NP = {F64: np.float64, F32: np.float32, I32: np.int32, torch.uint8: np.uint8}


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _p(t):
    return t.data_ptr() if t is not None else 0


def _raw(a):
    """A host array's bits as integers."""
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_raw(a), _raw(b))


def _ulps(a, b):
    """Distance in fp32 steps between finite arrays a and b (b fp64: first rounded to fp32)."""
    key = lambda x: np.where(_raw(x) < 0, np.int64(-(2 ** 31)) - _raw(x), _raw(x)).astype(np.int64)
    return np.abs(key(np.asarray(a, dtype=np.float32)) - key(np.asarray(b).astype(np.float32)))


class Guards:
    """Tensors that sit inside larger allocations; ``check()`` asserts that every border still holds its pattern."""

    def __init__(self, dev):
        self.dev, self.whole = dev, []

    def _view(self, shape, dtype):
        size = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        whole = torch.full((size + 2 * cases.GUARD_BYTES,), cases.GUARD_BYTE, dtype=torch.uint8, device=self.dev)
        self.whole.append(whole)
        return whole[cases.GUARD_BYTES:cases.GUARD_BYTES + size].view(dtype).view(*shape)

    def out(self, shape, dtype):
        """A pure output, every word the sentinel of its type."""
        t = self._view(shape, dtype)
        as_int, word = FILL[dtype]
        t.view(as_int).fill_(word)
        return t

    def put(self, a):
        """A tensor the op updates in place, holding the host array ``a``."""
        a = np.ascontiguousarray(a)
        t = self._view(a.shape, {v: k for k, v in NP.items()}[a.dtype.type])
        t.copy_(torch.from_numpy(a))
        return t

    def check(self):
        torch.cuda.synchronize(self.dev)
        for w in self.whole:
            lo, hi = w[:cases.GUARD_BYTES], w[-cases.GUARD_BYTES:]
            assert bool((lo == cases.GUARD_BYTE).all()) and bool((hi == cases.GUARD_BYTE).all()), "a write outside a buffer"
        return len(self.whole)


def _untouched(a):
    """Which words of a downloaded pure output still hold the sentinel."""
    a = np.ascontiguousarray(a)
    word = FILL[{v: k for k, v in NP.items()}[a.dtype.type]][1]
    return _raw(a) == word


# ---- 1. normals --------------------------------------------------------------------------------------------------------------

def _normals(g, dev, cloud, idx, k):
    n = cloud.shape[1]
    out, eig = g.out((1, n, 3), F32), g.out((1, n, 3), F64)
    _lib.call("icp_normals_kernel_wrapper", dev, 1, n, k, _p(cloud), _p(idx), _p(out), _p(eig))
    return out.cpu().numpy()[0], eig.cpu().numpy()[0]


def _direction_miss(got, want):
    g = got.astype(np.float64)
    length = np.linalg.norm(g, axis=1)
    assert (np.abs(length - 1.0) <= 2.0 ** -23).all()
    return 1.0 - np.abs(np.einsum("ni,ni->n", g / length[:, None], want))


@pytest.mark.parametrize("c", cases.normals_cases(), ids=lambda c: c["name"])
def test_normals_edges(cuda, c):
    x, n, k = c["xyz"], c["n"], c["k"]
    xd = _dev(x[None], cuda)
    idx, _ = registration.self_neighbours(xd, k)
    assert np.array_equal(idx.cpu().numpy()[0], model.knn(x, x, k + 1)[0])       # the lists are the model's
    g = Guards(cuda)
    got, eig = _normals(g, cuda, xd, idx, k)
    want, val, gap = model.normals(x, k)
    assert not _untouched(got).any() and not _untouched(eig).any()
    assert np.abs(eig - val).max() <= 64.0 * model.EPS64 * val[:, 2].max() and (np.diff(eig, axis=1) >= 0.0).all()
    assert (np.einsum("ni,ni->n", got.astype(np.float64), x.astype(np.float64)) <= 0.0).all()        # towards the origin
    worst = 0.0
    if c["edge"] == "rank_below":
        assert not want.any() and not _raw(got).any()                            # +0.0, every word
    elif c["edge"] in ("big", "nan"):
        use = gap >= model.GAP_MIN
        assert (~use).mean() <= model.GAP_CAP
        worst = (_direction_miss(got, want)[use] / (64.0 * model.EPS64 / gap[use])).max()
    else:
        worst = (_direction_miss(got, want) / (64.0 * model.EPS64 / gap)).max()
    if c["edge"] in ("planar", "origin"):
        assert (_direction_miss(got, np.tile(c["plane"], (n, 1))) <= 64.0 * model.EPS64 / gap).all()
    if c["edge"] == "planar":
        assert (got @ c["plane"].astype(np.float32) < 0.0).all()                 # n . y > 0 for every point: all flipped
    if c["edge"] == "origin":                                                    # n . y == 0: no flip, the solver's own sign
        x64 = x.astype(np.float64)
        for i in range(n):
            d = x64[idx.cpu().numpy()[0, i, 1:]] - x64[i]
            cov = [(d[:, a] * d[:, b]).sum() for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
            assert _same(got[i], model.eig3(cov)[1].astype(np.float32)) and got[i].tolist() == [0.0, 0.0, 1.0]
    if c["edge"] == "nan":                                                       # the lists of the clean cloud, one NaN point
        dirty, deig = _normals(g, cuda, _dev(cases.nan_cloud(c)[None], cuda), idx, k)
        hit = cases.nan_rows(c, idx.cpu().numpy()[0])
        assert hit[c["nan_point"]] and not _raw(dirty[hit]).any() and np.isnan(deig[hit]).any(axis=1).all()
        assert _same(dirty[~hit], got[~hit]) and _same(deig[~hit], eig[~hit])
    print("normals %s: worst miss / bound = %.3g, guard bands intact: %d" % (c["name"], worst, g.check()))
    assert worst <= 1.0
    _lib.synchronize(cuda)


# ---- 2. queries --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S, M, n", cases.QUERY_SHAPES)
def test_queries_edges(cuda, S, M, n):
    c = cases.queries_case(S, M, n)
    g = Guards(cuda)
    A, p, T = _dev(c["A"], cuda), _dev(c["p"], cuda), _dev(c["T"], cuda)
    eye = _dev(np.tile(np.eye(4), (S, M, 1, 1)), cuda)
    active = _dev(c["active"], cuda)
    worst = 0
    for t, th in ((None, None), (T, c["T"])):
        q = g.out((S, M, n, 3), F32)
        assert registration.queries(A, p, t, out=q) is q
        lock = q.cpu().numpy()
        assert not _untouched(lock).any()
        for s in range(S):
            worst = max(worst, int(_ulps(lock[s], model.queries(c["A"][s], c["p"][s], None if th is None else th[s])[0]).max()))
        q = g.out((S, M, n, 3), F32)
        registration.queries(A, p, t, active=active, out=q)
        masked = q.cpu().numpy()
        for s in range(S):
            if c["active"][s]:
                assert _same(masked[s], lock[s])
            else:
                assert _untouched(masked[s]).all()                               # the sentinel's bits, every word
    assert worst <= 1
    for t in (None, eye[:, 0].contiguous()):
        q = g.out((S, M, n, 3), F32)
        registration.queries(eye, p, t, out=q)
        assert _same(q.cpu().numpy(), np.ascontiguousarray(np.repeat(c["p"][:, None], M, axis=1)))
    print("queries S=%d M=%d n=%d: worst %d ulp, guard bands intact: %d" % (S, M, n, worst, g.check()))
    _lib.synchronize(cuda)


# ---- 3. accumulate -----------------------------------------------------------------------------------------------------------

def _accumulate(g, dev, c, t, active=None):
    S, M, n = c["S"], c["M"], c["n"]
    G = registration.groups(n)
    partial = g.out((S, G, 32), F64)
    args = (S, M, n) + tuple(_p(t[k]) for k in cases.ACC_KEYS) + (float(c["sigma"]), float(c["max_dist"]), _p(partial))
    if active is None:
        _lib.call("icp_accumulate_kernel_wrapper", dev, *args)
    else:
        _lib.call("icp_accumulate_masked_kernel_wrapper", dev, *args, _p(active))
    return partial.cpu().numpy()


@pytest.mark.parametrize("c", cases.accumulate_cases(), ids=lambda c: c["name"])
def test_accumulate_edges_row_by_row(cuda, c):
    S, n = c["S"], c["n"]
    t = {k: _dev(c[k], cuda) for k in cases.ACC_KEYS}
    g = Guards(cuda)
    got, again = _accumulate(g, cuda, c, t), _accumulate(g, cuda, c, t)
    assert got.shape == (S, (n + 255) // 256, 32) and _same(got, again)          # two runs: the same bits
    assert not _raw(got[:, :, 30:]).any()                                        # the padding words: +0.0 over the NaN
    worst = 0.0
    for s in range(S):
        want, mag = cases.case_groups(c, s)
        err = np.abs(got[s] - want)
        assert np.isfinite(got[s]).all()
        if (mag > 0).any():
            worst = max(worst, (err[mag > 0] / (1e-12 * mag[mag > 0])).max())
        assert (err <= 1e-12 * mag).all(), s
        assert np.array_equal(got[s][:, model.PAIRS], want[:, model.PAIRS])
        empty = want[:, model.PAIRS] == 0
        assert not _raw(got[s][empty]).any()                                     # a row without a pair: exact zeros
    mask = np.array([1, 0, 1], dtype=np.int32)
    masked = _accumulate(g, cuda, c, t, active=_dev(mask, cuda))
    assert _same(masked[0], got[0]) and _same(masked[2], got[2]) and not _raw(masked[1]).any()       # all 32 words of each row
    print("accumulate %s: worst err / (1e-12 sum|term|) = %.3g over %d rows, guard bands intact: %d"
          % (c["name"], worst, got.shape[0] * got.shape[1], g.check()))
    _lib.synchronize(cuda)


# ---- 4. solve ----------------------------------------------------------------------------------------------------------------

def _solve(g, dev, c, active=None, masked=False):
    S, G = c["S"], c["G"]
    T, status = g.put(c["T"]), g.put(c["status"])
    out = dict(iterations=g.out((S,), I32), pairs=g.out((S,), I32), cost=g.out((S,), F64), sum=g.out((S, 32), F64),
               delta=g.out((S, 6), F64))
    partial, words = _dev(c["partial"], dev), (_dev(active, dev) if masked else None)      # alive until the results are read
    args = (S, G, c["it"], _p(partial), c["damping"], c["threshold"], c["min_pairs"], _p(T), _p(status),
            _p(out["iterations"]), _p(out["pairs"]), _p(out["cost"]), _p(out["sum"]), _p(out["delta"]))
    if masked:
        _lib.call("icp_solve_masked_kernel_wrapper", dev, *args, _p(words))
    else:
        _lib.call("icp_solve_kernel_wrapper", dev, *args)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got.update(T=T.cpu().numpy(), status=status.cpu().numpy())
    return got


def _check_solve(c, got, active=None):
    """-> the worst err / bound of delta and T over the streams."""
    worst = 0.0
    finite = np.isfinite(c["rows"])
    assert np.array_equal(_raw(got["sum"])[finite], _raw(c["rows"])[finite]) and np.isnan(got["sum"][~finite]).all()
    for s in range(c["S"]):
        w = cases.solve_expected(c, s, active)
        what = (c["setting"], c["kinds"][s], s)
        assert int(got["status"][s]) == w["status"], what
        stepped = w["moved"] and w["status"] in (0, model.CONVERGED)
        if w["idle"]:
            assert got["iterations"][s] == 0 and got["pairs"][s] == 0 and _raw(got["cost"][s:s + 1])[0] == 0, what
        elif w["moved"]:
            assert got["iterations"][s] == c["it"] + 1 and got["pairs"][s] == int(c["rows"][s][model.PAIRS]), what
            assert _same(got["cost"][s:s + 1], c["rows"][s][model.COST:model.COST + 1]), what
        else:                                                                    # frozen earlier: the words are left alone
            assert _untouched(got["iterations"][s:s + 1]).all() and _untouched(got["pairs"][s:s + 1]).all(), what
            assert _untouched(got["cost"][s:s + 1]).all(), what
        scale, tol = np.abs(w["delta"]).max(), c["tol"][s]               # 1e-10 but for the general single pair (icp_cases)
        if stepped and scale > 0:
            worst = max(worst, np.abs(got["delta"][s] - w["delta"]).max() / (tol * scale))
            if c["kinds"][s] == "one_pair_general" and s < 5:
                print("general single pair, stream %d: relative error of delta %.3g, bound %.3g"
                      % (s, np.abs(got["delta"][s] - w["delta"]).max() / scale, tol))
        else:
            assert not got["delta"][s].any(), what                               # no step: zeros, written over the NaN
        assert _same(got["T"][s][3], c["T"][s][3]), what                         # row 3 is the caller's
        if stepped:
            # a step off by d moves a rotation entry by at most |d| and the translation by at most |d| (1 + |t|): the second
            # term is what the wider bound of the general single pair allows on top, zero for every other stream
            bound = 1e-10 * np.abs(w["T"][:3]).max() + 2.0 * (tol - 1e-10) * scale * (1.0 + np.abs(c["T"][s][:3, 3]).max())
            worst = max(worst, np.abs(got["T"][s][:3] - w["T"][:3]).max() / bound)
            if c["kinds"][s] == "zero_g":                                        # re-orthonormalised only
                assert np.abs(got["T"][s][:3] - c["T"][s][:3]).max() <= 1e-15, what
            if c["kinds"][s] == "step_345" and c["damping"] == 0.0:
                assert np.array_equal(got["delta"][s], cases.STEP_345), what     # no rounding on the way to the threshold
        else:
            assert _same(got["T"][s], c["T"][s]), what
    return worst


@pytest.mark.parametrize("G", cases.SOLVE_G)
@pytest.mark.parametrize("S", cases.SOLVE_S)
@pytest.mark.parametrize("setting", list(cases.SOLVE_SETTINGS))
def test_solve_edges(cuda, setting, S, G):
    c = cases.solve_case(setting, S, G)
    g = Guards(cuda)
    lock = _solve(g, cuda, c)
    worst = _check_solve(c, lock)
    masked = _solve(g, cuda, c, active=c["active"], masked=True)
    worst = max(worst, _check_solve(c, masked, active=c["active"]))
    ones = _solve(g, cuda, c, active=np.ones((S,), dtype=np.int32), masked=True)
    for key in lock:
        assert _same(ones[key], lock[key]), key                                  # all active: the lock-step bits
    if c["it"] > 0:                                                              # the words are read in iteration 0 only
        late = _solve(g, cuda, c, active=np.zeros((S,), dtype=np.int32), masked=True)
        for key in lock:
            assert _same(late[key], lock[key]), key
    print("solve %s S=%d G=%d: worst err / (1e-10 scale) = %.3g, guard bands intact: %d" % (setting, S, G, worst, g.check()))
    assert worst <= 1.0
    _lib.synchronize(cuda)


# ---- 5. begin, push, gated push ------------------------------------------------------------------------------------------------

STATE = ("map_xyz", "map_normals", "map_ws", "A", "R", "live", "cursor")


def _compare(dev_state, maps, what, keys=STATE):
    want = maps.state()
    for k in keys:
        assert _same(dev_state[k].cpu().numpy().reshape(want[k].shape), want[k]), (what, k)


@pytest.mark.parametrize("M", cases.PUSH_M)
def test_begin_every_word_combination(cuda, M):
    S = 3
    first = cases.Maps(S, M, 64, 7)
    first.cursor[:] = (M - 1, 0, M // 2)
    keys = ("A", "R", "live", "cursor")
    g = Guards(cuda)
    state = {k: g.put(first.state()[k]) for k in keys}
    pristine = {k: v.clone() for k, v in state.items()}
    armed_words = g.put(np.zeros((S,), dtype=np.int32))                         # the kernel writes it: between guard bands too
    calls = 0
    for with_armed in (True, False):
        for w in cases.words(3 if with_armed else 2):
            for k in keys:
                state[k].copy_(pristine[k])
            maps = copy.deepcopy(first)
            word = _dev(np.ascontiguousarray(w.T), cuda)                         # rows: active, restart[, armed]
            armed = None
            if with_armed:
                armed = armed_words
                armed.copy_(word[2])
            registration.begin(word[0], word[1], state["A"], state["R"], state["live"], state["cursor"], armed=armed)
            host_armed = w[:, 2].copy() if with_armed else None
            maps.begin(w[:, 0], w[:, 1], host_armed)
            _compare(state, maps, w.tolist(), keys)
            if with_armed:
                assert armed.tolist() == host_armed.tolist(), w.tolist()
            calls += 1
    print("begin M=%d: %d calls, guard bands intact: %d" % (M, calls, g.check()))
    _lib.synchronize(cuda)


def _push(dev, S, M, n, f, state, active=None, insert=None, gated=False):
    args = (S, M, n, _p(f["T"]), _p(f["cloud"]), _p(f["normals"]), _p(f["stage_ws"])) + tuple(_p(state[k]) for k in STATE)
    if gated:
        _lib.call("keyframe_icp_push_kernel_wrapper", dev, *args, _p(active), _p(insert))
    elif active is not None:
        _lib.call("icp_map_push_masked_kernel_wrapper", dev, *args, _p(active))
    else:
        _lib.call("icp_map_push_kernel_wrapper", dev, *args)


@pytest.mark.parametrize("M", cases.PUSH_M)
@pytest.mark.parametrize("n", cases.PUSH_N)
def test_push_every_word_combination(cuda, n, M):
    S = 3
    maps = cases.Maps(S, M, n, 11)
    maps.cursor[:] = (-1, M, M // 2)                                             # two words outside [0, M): clamped
    lib = _lib.load()
    assert maps.ws().size == lib.knn_point_build_bytes(S * M, n)
    g = Guards(cuda)
    state = {k: g.put(v) for k, v in maps.state().items()}
    frames = [cases.frame(S, n, k) for k in range(4)]
    assert frames[0]["stage_ws"].size == lib.knn_point_build_bytes(S, n)
    staged = [{k: _dev(v, cuda) for k, v in f.items()} for f in frames]
    calls = 0

    def one(active, insert, gated):
        nonlocal calls
        k = calls % len(frames)
        _push(cuda, S, M, n, staged[k], state, None if active is None else _dev(active, cuda),
              None if insert is None else _dev(insert, cuda), gated)
        maps.push(frames[k]["T"], frames[k], active, insert)
        _compare(state, maps, (calls, active, insert, gated))
        calls += 1

    for w in cases.words(2):                                                     # the gated push: active x insert per stream
        one(w[:, 0].copy(), w[:, 1].copy(), True)
    for w in cases.words(1):
        one(None, w[:, 0].copy(), True)                                          # gated, lock step
        one(w[:, 0].copy(), None, False)                                         # masked
    for _ in range(3):
        one(None, None, False)                                                   # lock step
    assert ((maps.cursor >= 0) & (maps.cursor < M)).all()                        # every stream has inserted: in range again
    print("push n=%d M=%d: %d calls, every array bit for bit, guard bands intact: %d" % (n, M, calls, g.check()))
    _lib.synchronize(cuda)


def test_push_clamps_the_cursor_and_wraps_a_map_of_one(cuda):
    S, n = 3, 64
    for M, cursor, slots, after in ((4, (-1, 4, 9), (0, 3, 3), (1, 0, 0)), (1, (-1, 1, 0), (0, 0, 0), (0, 0, 0))):
        maps = cases.Maps(S, M, n, 13)
        maps.cursor[:] = cursor
        g = Guards(cuda)
        state = {k: g.put(v) for k, v in maps.state().items()}
        for k in range(3):                                                       # M = 1: three pushes, the one slot every time
            f = cases.frame(S, n, 20 + k)
            _push(cuda, S, M, n, {key: _dev(v, cuda) for key, v in f.items()}, state)
            maps.push(f["T"], f)
            _compare(state, maps, (M, k))
            if k == 0:
                assert state["cursor"].tolist() == list(after)
                for s in range(S):
                    assert _same(state["map_xyz"][s, slots[s]].cpu().numpy(), f["cloud"][s])
            if M == 1:
                assert state["cursor"].tolist() == [0, 0, 0] and state["live"].tolist() == [[1]] * S
                assert _same(state["A"].cpu().numpy(), np.tile(np.eye(4), (S, 1, 1, 1)))
                assert _same(state["map_xyz"][:, 0].cpu().numpy(), f["cloud"])
        g.check()
    _lib.synchronize(cuda)
