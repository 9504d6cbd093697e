"""``graphed.PipelinedForward`` on the native library's stream set (csrc/pipeline.hip, ``pipe_streams.StreamSet``): the
poses are bit for bit those of ``GraphedForward`` and of the torch-stream path, at every depth, with the streams reused
by a second pipeline, and with inputs produced on a side stream.  Batch 2 at 4096 points, the size of the other
pipelined-forward tests (tests/test_gpu_fused.py)."""
import ctypes

import pytest
import torch

import pwclonet_pylidarslam_amd

from oracle import params
from pwclonet_pylidarslam_amd import _lib, pipe_streams, synthetic
from pwclonet_pylidarslam_amd.graphed import GraphedForward, PipelinedForward
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet

pytestmark = pytest.mark.gpu

EINVAL = 10001
CALLS = 8


@pytest.fixture(scope="module")
def ctx(cuda):
    """The net, three distinct input pairs and their ``GraphedForward`` poses (checked against the eager forward)."""
    net = PWCLONet(dict(num_input_channels=3, sequence_len=2, device=str(cuda), scalar_last=False, log_mode="none"))
    params.fill_state_dict(net.state_dict())
    net = net.to(cuda).eval()
    net.prepare_fused()
    pc1, pc2, _, _ = synthetic.kitti_like_pair(41, 4096, 2)
    x1 = torch.from_numpy(pc1[:, :, :3]).permute(0, 2, 1).contiguous().to(cuda)
    x2 = torch.from_numpy(pc2[:, :, :3]).permute(0, 2, 1).contiguous().to(cuda)
    inputs = [(x1, x2), (x2, x1), (x1.flip(0).contiguous(), x2)]
    g = GraphedForward(net)
    refs = [g(a, b).clone() for a, b in inputs]
    with torch.no_grad():
        eager = [net(a, None, b, None)[0].clone() for a, b in inputs]
    torch.cuda.synchronize(cuda)
    for r, e in zip(refs, eager):
        assert torch.equal(r, e)
    assert not torch.equal(refs[0], refs[1]) and not torch.equal(refs[0], refs[2]) and not torch.equal(refs[1], refs[2])
    return dict(net=net, inputs=inputs, refs=refs, dev=cuda)


def _run(pipe, ctx, calls=CALLS):
    """`calls` consecutive calls over the three inputs, nothing waited for in between: every output is cloned on its
    slot's stream behind the replay (the slot's buffer is overwritten `depth` calls later).  -> [(clone, input index)]"""
    got, first = [], pipe._calls
    for c in range(calls):
        k = c % 3
        out, slot = pipe(*ctx["inputs"][k])
        assert slot == (first + c) % len(pipe.slots)
        assert pipe._where[slot] is pipe.streams[(first + c) % pipe._lanes]
        with torch.cuda.stream(pipe._where[slot]):
            got.append((out.clone(), k))
    pipe.wait_all()
    return got


def _check(got, ctx, what):
    for c, (pose, k) in enumerate(got):
        assert torch.equal(pose, ctx["refs"][k]), "%s: call %d (input %d) differs from GraphedForward" % (what, c, k)


@pytest.fixture(scope="module")
def native4(ctx):
    assert pipe_streams.mode() == "native"                       # the default of the process that runs the suite
    pipe = PipelinedForward(ctx["net"], depth=4)
    got = _run(pipe, ctx)
    return pipe, got


def test_depth4_on_the_native_set_is_graphed_forward(ctx, native4):
    pipe, got = native4
    assert pipe._set is not None and pipe._set.n == 4
    assert all(isinstance(s, torch.cuda.ExternalStream) for s in pipe.streams)
    # every slot has a stream where the process has more hardware queues than slots; else queues - 1 streams carry them
    q = pwclonet_pylidarslam_amd.hw_queues() or 4
    assert pipe._lanes == pipe_streams.lanes(4) == (4 if q > 4 else q - 1)
    _check(got, ctx, "native set, depth 4")
    for slot in range(4):                                        # per-slot completion: recorded, reached, waitable
        assert pipe.events[slot].query()
        pipe.wait(slot)


def test_depth4_on_torch_streams_is_the_same(ctx, native4, monkeypatch):
    monkeypatch.setattr(pipe_streams, "_mode", "torch")         # what PWCLO_PIPE_STREAMS=torch selects for a process
    pipe = PipelinedForward(ctx["net"], depth=4)
    got = _run(pipe, ctx)
    assert pipe._set is None and not any(isinstance(s, torch.cuda.ExternalStream) for s in pipe.streams)
    assert pipe._lanes == 4                                      # one torch stream per slot, as before the set existed
    assert all(isinstance(e, torch.cuda.Event) for e in pipe.events)
    _check(got, ctx, "torch streams, depth 4")
    for (a, ka), (b, kb) in zip(got, native4[1]):
        assert ka == kb and torch.equal(a, b)


@pytest.mark.parametrize("depth", [1, 3])
def test_other_depths_on_the_native_set(ctx, depth):
    pipe = PipelinedForward(ctx["net"], depth=depth)
    got = _run(pipe, ctx)
    assert pipe._set is not None and pipe._set.n == depth and len(pipe.streams) == depth
    _check(got, ctx, "native set, depth %d" % depth)


def test_a_second_pipeline_reuses_the_streams(ctx):
    first = PipelinedForward(ctx["net"], depth=4)
    _check(_run(first, ctx, calls=4), ctx, "first pipeline")
    handles = [s.cuda_stream for s in first.streams]
    second = PipelinedForward(ctx["net"], depth=4, streams=first.streams)
    del first                                                    # the wrappers keep the set alive
    got = _run(second, ctx)
    assert [s.cuda_stream for s in second.streams] == handles and second._set is None
    assert second._lanes == pipe_streams.lanes(4)                # native streams: the same rotation as their first user
    _check(got, ctx, "second pipeline on the first one's streams")


def test_the_four_streams_are_distinct_and_not_the_callers(ctx, native4):
    pipe, _ = native4
    handles = [s.cuda_stream for s in pipe.streams]
    assert handles == [pipe._set.handle(i) for i in range(4)]
    assert len(set(handles)) == 4 and 0 not in handles
    assert torch.cuda.current_stream(ctx["dev"]).cuda_stream not in handles


def test_create_destroy_create(ctx):
    lib = _lib.load()
    a = pipe_streams.StreamSet(4, ctx["dev"])
    old, p = a._handle, ctypes.c_void_p()
    assert lib.pwclo_stream_set_size(old) == 4
    assert lib.pwclo_stream_set_stream(old, 4, ctypes.byref(p)) == EINVAL      # one past the set's last stream
    assert lib.pwclo_stream_set_stream(old, 3, ctypes.byref(p)) == 0 and p.value
    a.close()
    assert lib.pwclo_stream_set_size(old) == -EINVAL                            # destroyed: refused from now on
    assert lib.pwclo_stream_set_stream(old, 0, ctypes.byref(p)) == EINVAL
    assert lib.pwclo_stream_set_destroy(old) == EINVAL
    b = pipe_streams.StreamSet(4, ctx["dev"])
    assert b._handle > old and len({b.handle(i) for i in range(4)}) == 4
    x = torch.zeros(1024, device=ctx["dev"])
    torch.cuda.synchronize(ctx["dev"])
    new = b._handle
    with torch.cuda.stream(b.wrap(2)):
        y = x + 1
    ev = b.record(5, 2)
    b.synchronize()
    assert ev.query() and float(y.sum()) == 1024.0
    b.close()
    assert lib.pwclo_stream_set_size(new) == -EINVAL


def test_inputs_filled_on_a_side_stream_are_honoured(ctx, native4):
    """The caller fills the input buffers on ITS stream right before the call; the slot's stream must wait for that."""
    pipe, _ = native4
    dev = ctx["dev"]
    (a0, b0), (a2, b2) = ctx["inputs"][0], ctx["inputs"][2]
    xa, xb = a2.clone(), b2.clone()                              # start as input 2: a missed wait would give ITS pose
    busy = torch.randn(2048, 2048, device=dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        for _ in range(8):                                       # the fill sits behind some milliseconds of work
            busy = busy @ busy * 1e-3
        xa.copy_(a0)
        xb.copy_(b0)
        out, slot = pipe(xa, xb)
    pipe.wait(slot)
    assert torch.equal(out, ctx["refs"][0])
    torch.cuda.synchronize(dev)
