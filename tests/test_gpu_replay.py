"""``stream_engine.Replay`` on the device, alone: the body is one in-place add on 64 elements, no
kernel of the project is involved.  A sum that grows by exactly one increment per call shows that an eager call, a capture
plus its replay, and a replay each ran the body once."""
import pytest
import torch

from pwclonet_pylidarslam_amd.stream_engine import Replay

pytestmark = pytest.mark.gpu
N = 64


def _counter(step):
    x = torch.zeros(N, dtype=torch.float64, device="cuda")
    return x, lambda: x.add_(step)


def _holds(x, value):
    return torch.equal(x, torch.full((N,), float(value), dtype=torch.float64, device="cuda"))


def test_call_0_is_eager_call_1_captures_and_later_calls_replay_it():
    x, body = _counter(3.0)
    r = Replay(True)
    r.run(body, x.device)
    assert r.calls == 1 and r.captures == 0 and r.graph() is None and r.graphs == {} and _holds(x, 3)
    r.run(body, x.device)
    g = r.graph()
    assert r.calls == 2 and r.captures == 1 and isinstance(g, torch.cuda.CUDAGraph) and _holds(x, 6)
    for k in range(3, 6):
        r.run(body, x.device)
        assert r.calls == k and r.captures == 1 and r.graph() is g and list(r.graphs) == [None] and _holds(x, 3 * k)


def test_every_key_has_a_graph_of_its_own():
    x, add_one = _counter(1.0)
    add_ten = lambda: x.add_(10.0)
    r = Replay(True)
    r.run(add_one, x.device, key="one")                 # eager
    want = 1
    for k, (key, body, step) in enumerate([("one", add_one, 1), ("ten", add_ten, 10)] * 3):
        r.run(body, x.device, key=key)
        want += step
        assert _holds(x, want) and r.captures == min(k + 1, 2) and r.calls == k + 2
    one, ten = r.graph("one"), r.graph("ten")
    assert one is not None and ten is not None and one is not ten and r.graph() is None and set(r.graphs) == {"one", "ten"}
    # a replay runs what its key captured, not the body handed in with it
    r.run(add_ten, x.device, key="one")
    assert _holds(x, want + 1) and r.captures == 2 and r.graph("one") is one


def test_drop_forgets_the_graphs_and_keeps_the_count():
    x, body = _counter(2.0)
    r = Replay(True)
    for _ in range(3):
        r.run(body, x.device, key=7)
    old = r.graph(7)
    assert r.captures == 1 and old is not None
    r.drop()
    assert r.graphs == {} and r.graph(7) is None and r.captures == 1 and r.calls == 3 and _holds(x, 6)
    r.run(body, x.device, key=7)                        # captures again; no second eager call
    assert r.captures == 2 and r.calls == 4 and r.graph(7) is not None and r.graph(7) is not old and _holds(x, 8)
    r.run(body, x.device, key=7)
    assert r.captures == 2 and r.calls == 5 and _holds(x, 10)


def test_without_graph_nothing_is_ever_captured():
    x, body = _counter(5.0)
    r = Replay(False)
    for k in range(1, 5):
        r.run(body, x.device, key=k % 2)
        assert r.calls == k and r.captures == 0 and r.graphs == {} and _holds(x, 5 * k)


def test_a_body_that_raises_on_call_0_counts_nothing():
    x, body = _counter(1.0)

    def broken():
        raise ValueError("refused before any launch")
    r = Replay(True)
    with pytest.raises(ValueError, match="refused before any launch"):
        r.run(broken, x.device)
    assert r.calls == 0 and r.captures == 0 and r.graphs == {}
    r.run(body, x.device)                               # so this one is call 0: eager
    assert r.calls == 1 and r.captures == 0 and r.graph() is None and _holds(x, 1)
