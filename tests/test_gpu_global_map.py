"""GPU tests of the global map's kernels against the NumPy model of tests/global_map_model.py.  Every
comparison is exact: the points' bits, the sources, the totals and the counts."""
import numpy as np
import pytest
import torch

import global_map_cases as C
import global_map_model as M
import loop_closure_cases as LC
from pwclonet_pylidarslam_amd import _lib, global_map
from pwclonet_pylidarslam_amd.global_map import GlobalMap

pytestmark = pytest.mark.gpu
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _same(got, want, what=None):
    points, source, total = got
    assert int(total) == want[2], (what, int(total), want[2])
    assert tuple(points.shape) == want[0].shape and tuple(source.shape) == want[1].shape, (what, points.shape, want[0].shape)
    assert np.array_equal(source.cpu().numpy(), want[1]), what
    assert np.array_equal(_bits(points.cpu().numpy()), _bits(want[0])), what


def _build(cuda, clouds, X, v, lengths=None, capacity=None):
    return global_map.build(torch.from_numpy(clouds).to(cuda), torch.from_numpy(X).to(cuda), v,
                            None if lengths is None else torch.from_numpy(lengths).to(cuda), capacity)


# ---- the op ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, n, K, v", C.TABLE)
def test_op_equals_the_model(cuda, name, n, K, v):
    clouds, X, lengths = C.case(name, n, K, v)
    want = M.build(clouds, X, v, lengths=lengths)
    _same(_build(cuda, clouds, X, v, lengths), want)


@pytest.mark.parametrize("name", ["uniform", "dense", "marker", "partial"])
def test_capacity_drops_the_last_winners_and_total_is_not_clamped(cuda, name):
    clouds, X, lengths = C.case(name, 257, 3, 0.3)
    total = M.build(clouds, X, 0.3, lengths=lengths)[2]
    assert 2 < total < 3 * 257
    for cap in (1, total - 1, total, total + 1, 3 * 257):
        got = _build(cuda, clouds, X, 0.3, lengths, capacity=cap)
        _same(got, M.build(clouds, X, 0.3, lengths=lengths, capacity=cap), cap)
        assert got[0].shape[0] == min(cap, total) and got[2] == total


def test_revisit_scene_at_the_chain_and_at_the_true_path(cuda):
    r = LC.revisit()
    frames = np.ascontiguousarray(r["frames"][:, 0])
    path = np.stack(r["path"])
    true = np.linalg.inv(path[0]) @ path
    chain = [np.eye(4)]
    for k in range(1, 40):
        chain.append(chain[-1] @ r["chain"][k])
    chain = np.stack(chain)
    for X, total in ((true, 5875), (chain, 8285)):
        got = _build(cuda, frames, X, 0.3)
        assert got[2] == total
        _same(got, M.build(frames, X, 0.3))


# ---- the class ---------------------------------------------------------------------------------------------------------

def _stream_state(gm, s):
    p, src = gm.points(s), gm.sources(s)
    return p.clone(), src.clone(), int(gm.totals()[s])


@pytest.mark.parametrize("stride, max_new, MK, capacity", [(1, 1, 8, 400), (3, 2, 8, None), (1, 2, 16, 500)])
def test_stateful_schedule(cuda, stride, max_new, MK, capacity):
    S, n, v = 3, 96, 0.3
    calls = C.schedule(S, n)
    X0, X1 = C.trajectory(S, 16, seed=9), C.trajectory(S, 16, seed=10)
    X = torch.from_numpy(X0).to(cuda)
    kw = dict(voxel_size=v, max_keyframes=MK, capacity=capacity, stride=stride, max_new=max_new, device=cuda)
    gm, eager = GlobalMap(S, n, **kw), GlobalMap(S, n, graph=False, **kw)
    cap = gm.capacity

    def run(until, record=None):
        banks = [M.Bank(n, MK, stride, max_new) for _ in range(S)]
        for c, (clouds, ids, active, restart, lengths) in enumerate(calls[:until]):
            if c == 5:                                           # every banked keyframe of stream 0 pending again
                for g in (gm, eager):
                    g.invalidate([0])
                banks[0].invalidate()
                assert len(banks[0].frames) - banks[0].built >= (3 if stride == 1 else 2)
            dev = lambda a: torch.from_numpy(a).to(cuda)
            for g in (gm, eager):
                g.advance(dev(clouds), dev(ids), X, active=dev(active), restart=dev(restart), lengths=dev(lengths))
            for s in range(S):
                if active[s]:
                    banks[s].advance(clouds[s], int(ids[s]), int(lengths[s]), bool(restart[s]))
                got = _stream_state(gm, s)
                _same(got, banks[s].map(X.cpu().numpy()[:, s], v, cap), (c, s))
                _same(_stream_state(eager, s), banks[s].map(X.cpu().numpy()[:, s], v, cap), (c, s, "eager"))
                assert int(gm.counts()[s]) == len(banks[s].frames) and int(gm.built()[s]) == banks[s].built, (c, s)
                if record is not None:
                    record.append(got)
            for name in ("state", "overflow"):                                   # eager equals replay
                assert torch.equal(gm.bufs[name], eager.bufs[name]), (c, name)
            for s in range(S):
                k = len(banks[s].frames)
                for name in ("bank_frame", "bank_len", "bank_cloud"):
                    assert torch.equal(gm.bufs[name][s, :k], eager.bufs[name][s, :k]), (c, s, name)
                assert gm.bufs["bank_frame"][s, :k].tolist() == banks[s].frames, (c, s)
                assert gm.bufs["bank_len"][s, :k].tolist() == banks[s].lengths, (c, s)
        return banks

    first = []
    banks = run(len(calls), first)
    assert gm.captures == 1 and eager.captures == 0
    assert gm.overflowed() == eager.overflowed() == any(b.overflow for b in banks) == (stride == 1 and MK == 8)
    caught = [b.built == len(b.frames) for b in banks]                           # nothing pending any more
    assert sum(caught) >= 2 and (max_new == 1 or all(caught))                    # (one a call never catches up while banking)
    if stride == 1 and MK == 8:                                                  # the full bank kept its eight keyframes
        assert int(gm.counts()[0]) == 8 and banks[0].frames == list(range(8))

    # advance x k equals one rebuild
    before = [_stream_state(gm, s) for s in range(S)]
    gm.rebuild(X)
    for s in range(S):
        banks[s].rebuild()
        after = _stream_state(gm, s)
        _same(after, banks[s].map(X0[:, s], v, cap), ("rebuild at the same poses", s))
        if caught[s]:
            assert after[2] == before[s][2] and torch.equal(after[0], before[s][0]) and torch.equal(after[1], before[s][1]), s

    # a rebuild at other poses (the same buffer: the same graphs), then an advance that appends to it
    X.copy_(torch.from_numpy(X1))
    gm.rebuild(X)
    for s in range(S):
        _same(_stream_state(gm, s), banks[s].map(X1[:, s], v, cap), ("rebuild", s))
    assert gm.captures == 2
    rng = np.random.default_rng(3)
    cloud = rng.uniform(-1.5, 1.5, (S, n, 3)).astype(F)
    ids = np.array([len(b.frames) * stride for b in banks], dtype=np.int32)
    gm.advance(torch.from_numpy(cloud).to(cuda), ids, X)
    for s in range(S):
        old = banks[s].map(X1[:, s], v)
        banks[s].advance(cloud[s], int(ids[s]))
        new = banks[s].map(X1[:, s], v)
        assert new[2] >= old[2] and np.array_equal(_bits(new[0][:old[2]]), _bits(old[0]))
        _same(_stream_state(gm, s), banks[s].map(X1[:, s], v, cap), ("append", s))
    assert gm.captures == 2

    # the same object again after reset: the same bits, no new graph
    gm.reset()
    eager.reset()
    X.copy_(torch.from_numpy(X0))
    assert gm.counts().tolist() == [0] * S and gm.totals().tolist() == [0] * S and not gm.overflowed()
    again = []
    run(5, again)
    for a, b in zip(again, first):
        assert a[2] == b[2] and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert gm.captures == 2


def test_reset_of_one_stream_and_an_idle_stream_keep_the_others(cuda):
    S, n, v = 2, 65, 0.3
    X = torch.from_numpy(C.trajectory(S, 4)).to(cuda)
    gm = GlobalMap(S, n, voxel_size=v, max_keyframes=4, device=cuda)
    rng = np.random.default_rng(1)
    clouds = rng.uniform(-1, 1, (3, S, n, 3)).astype(F)
    for f in range(2):
        gm.advance(torch.from_numpy(clouds[f]).to(cuda), [f, f], X)
    keep = _stream_state(gm, 1)
    words = {k: t.clone() for k, t in gm.bufs.items()}
    gm.reset([0])
    gm.advance(torch.from_numpy(clouds[2]).to(cuda), [0, 2], X, active=[1, 0])
    now = _stream_state(gm, 1)
    assert now[2] == keep[2] and torch.equal(now[0], keep[0]) and torch.equal(now[1], keep[1])
    for name in ("keys", "rows", "slots", "bank_cloud", "bank_frame", "bank_len", "points", "source"):
        assert torch.equal(gm.bufs[name][1], words[name][1]), name                # an idle stream keeps every word
    assert torch.equal(gm.bufs["state"][1, :4], words["state"][1, :4])
    _same(_stream_state(gm, 0), M.build(clouds[2, 0][None], X[:, 0].cpu().numpy(), v), "after reset")
    assert gm.counts().tolist() == [1, 2]


# ---- the library's own refusals ----------------------------------------------------------------------------------------

def test_library_refuses_bad_arguments_before_any_launch(cuda):
    S, MK, n, cap = 2, 4, 65, 100
    b = global_map._buffers(S, MK, n, cap, cuda)
    for t in b.values():
        t.fill_(7)
    saved = {k: t.clone() for k, t in b.items()}
    X = torch.eye(4, dtype=torch.float64, device=cuda).expand(3, S, 4, 4).contiguous()
    p = lambda name: b[name].data_ptr()
    ids = torch.zeros(S, dtype=torch.int32, device=cuda)

    def begin(S=S, MK=MK, n=n, stride=1, E=1, mode=0, state=p("state"), frame_id=ids.data_ptr()):
        return ("global_map_begin_kernel_wrapper", S, MK, n, stride, E, mode, 0, 0, frame_id, 0, state, p("bank_frame"),
                p("bank_len"), p("overflow"))

    def insert(S=S, MK=MK, n=n, E=1, voxel=0.3, X=X.data_ptr(), frames=3, keys=p("keys")):
        return ("global_map_insert_kernel_wrapper", S, MK, n, E, voxel, X, frames, p("bank_cloud"), p("bank_frame"),
                p("bank_len"), p("state"), keys, p("rows"), p("slots"))

    def write(capacity=cap, points=p("points"), E=1, frames=3):
        return ("global_map_write_kernel_wrapper", S, MK, n, E, capacity, X.data_ptr(), frames, p("bank_cloud"),
                p("bank_frame"), p("bank_len"), p("state"), p("keys"), p("rows"), p("slots"), p("blocks"), points, p("source"))

    bad = [begin(S=0), begin(S=1025), begin(MK=0), begin(MK=65536), begin(n=0), begin(MK=1024, n=(1 << 19) + 1),
           begin(stride=0), begin(E=0), begin(E=MK + 1), begin(mode=2), begin(state=0), begin(frame_id=0),
           insert(voxel=0.0), insert(voxel=-0.3), insert(voxel=float("nan")), insert(voxel=float("inf")), insert(E=0),
           insert(E=MK + 1), insert(X=0), insert(frames=0), insert(keys=0), insert(keys=p("keys") + 4), insert(S=0),
           write(capacity=0), write(capacity=MK * n + 1), write(points=0), write(E=0), write(frames=0),
           ("global_map_push_kernel_wrapper", S, MK, n, 0, p("state"), p("bank_cloud")),
           ("global_map_clear_kernel_wrapper", S, MK, n, p("state"), 0, p("rows")),
           ("global_map_clear_kernel_wrapper", S, 0, n, p("state"), p("keys"), p("rows")),
           ("global_map_count_kernel_wrapper", S, MK, n, 1, p("bank_len"), p("state"), p("keys"), p("rows"), p("slots"), 0),
           ("global_map_scan_kernel_wrapper", S, MK, n, 0, p("blocks")),
           ("global_map_end_kernel_wrapper", 0, p("state")), ("global_map_end_kernel_wrapper", S, 0)]
    lib = _lib.load()
    for call in bad:
        with pytest.raises(RuntimeError, match=call[0].replace("_kernel_wrapper", "")):
            _lib.call(call[0], cuda, *call[1:])
        assert lib.pwclo_last_error() == 0                                       # the check cleared it
    torch.cuda.synchronize()
    for k, t in b.items():
        assert torch.equal(t, saved[k]), k                                       # no launch wrote anything
