"""In-place refresh of the packed eval-mode weights (csrc/pack_refresh.hip, pack_plan.PackPlan, ``FusedPWCLONet.refresh``,
``PWCLONet.refresh_fused`` / ``prepare_fused(persistent=True)``).  The bar everywhere is BIT equality with what the
existing packer produces (``pack_layer(*fold_conv_bn(layer), ...)``, a freshly constructed ``FusedPWCLONet``), with every
buffer address and object identity unchanged, so captured graphs keep replaying -- with the new weights."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import params
from pwclonet_pylidarslam_amd import fused, pack_plan, synthetic
from pwclonet_pylidarslam_amd.graphed import GraphedForward
from pwclonet_pylidarslam_amd.odometry import StreamingOdometry
from pwclonet_pylidarslam_amd.pointnet2_ops import pytorch_utils as pt
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16x3", "bf16"]
WFMT = {"f32": fused.WFMT_F32, "bf16x3": fused.WFMT_BF16X3, "bf16": fused.WFMT_BF16}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _net(dev, fill=""):
    net = PWCLONet(dict(num_input_channels=3, sequence_len=2, device=str(dev), scalar_last=False, log_mode="none"))
    net = net.to(dev).eval()
    _refill(net, fill)
    return net


def _refill(net, tag):
    """Overwrite every parameter and BatchNorm buffer IN PLACE with the deterministic fill keyed ``tag + name``."""
    with torch.no_grad():
        for k, v in net.state_dict().items():
            val = torch.from_numpy(np.array(params.fill_value(tag + k, v.shape))).reshape(v.shape)
            v.copy_(val.to(v.dtype))


def _pair(dev, n=1024, b=2):
    pc1, pc2 = synthetic.uniform_pair(4242, n, b)
    cm = lambda pc: torch.from_numpy(pc[:, :, :3]).permute(0, 2, 1).contiguous().to(dev)
    return cm(pc1), cm(pc2)


def _assert_buffers_equal(fs, fresh):
    a, b = fs.packed_buffers(), fresh.packed_buffers()
    assert sorted(a) == sorted(b) and len(a) >= 20
    for name in a:
        assert torch.equal(_bits(a[name]), _bits(b[name])), name


# ---- the kernel against pack_layer(*fold_conv_bn(layer), ...) -----------------------------------------------------------

def _layer(cin, cout, dev, seed, bn=True, var=None):
    g = torch.Generator().manual_seed(seed)
    layer = pt.Conv2d(cin, cout, bn=bn).eval()
    u = lambda shape, lo, hi: torch.rand(shape, generator=g) * (hi - lo) + lo
    with torch.no_grad():
        layer.conv.weight.copy_(u(layer.conv.weight.shape, -0.5, 0.5))
        if layer.conv.bias is not None:
            layer.conv.bias.copy_(u((cout,), -0.5, 0.5))
        if bn:
            b = layer.bn.bn
            b.weight.copy_(u((cout,), 0.5, 1.5))
            b.bias.copy_(u((cout,), -1, 1))
            b.running_mean.copy_(u((cout,), -1, 1))
            b.running_var.copy_(var if var is not None else u((cout,), 0.5, 2))
    return layer.to(dev)


def _cases(dev):
    """[(name, layer, pack(w, b, wfmt) -> packed)]: the smallest layers that reach each branch of the kernel."""
    F = fused
    wide_var = torch.logspace(-6, 3, 32)                                     # running_var from 1e-6 to 1e3
    return [
        ("kmajor_cout8", _layer(6, 8, dev, 1),
         lambda w, b, f: F.pack_layer(w, b, F.kstep_major_map(6), 1, f, kmajor_out=True)),
        ("kmajor_cout16", _layer(8, 16, dev, 2),
         lambda w, b, f: F.pack_layer(w, b, F.kstep_major_map(8), 1, f, kmajor_out=True)),
        ("kstep3_slice_zero_bias", _layer(19, 32, dev, 3),
         lambda w, b, f: F.pack_layer(F._cols(w, 0, 3), F._zeros_like_bias(w), F.kstep_major_map(3), 2, f)),
        ("kstep6", _layer(6, 8, dev, 4), lambda w, b, f: F.pack_layer(w, b, F.kstep_major_map(6), 1, f)),
        ("kstep10_slice", _layer(42, 32, dev, 5),
         lambda w, b, f: F.pack_layer(F._cols(w, 0, 10), F._zeros_like_bias(w), F.kstep_major_map(10), 2, f)),
        ("16to16", _layer(16, 16, dev, 6), lambda w, b, f: F.pack_layer(w, b, F.chain_map(16, 1), 1, f)),
        ("32to24_padded_out", _layer(32, 24, dev, 7), lambda w, b, f: F.pack_layer(w, b, F.chain_map(32, 2), 2, f)),
        ("48to16_odd_nbi", _layer(48, 16, dev, 8), lambda w, b, f: F.pack_layer(w, b, F.chain_map(48, 3), 1, f)),
        ("pre_job_form", _layer(35, 24, dev, 9),                             # columns 3.., rows padded 24 -> 32, zero bias
         lambda w, b, f: F.pack_layer(F._pad_rows(F._cols(w, 3), 32), F._pad_rows(F._zeros_like_bias(w), 32),
                                      list(range(32)), None, f)),
        ("middle_slice_with_bias", _layer(42, 32, dev, 10),
         lambda w, b, f: F.pack_layer(F._cols(w, 10, 26), b, list(range(16)), None, f)),
        ("conv_bias_no_bn", _layer(32, 32, dev, 11, bn=False), lambda w, b, f: F.pack_layer(w, b, F.chain_map(32, 2), 2, f)),
        ("wide_running_var", _layer(32, 32, dev, 12, var=wide_var),
         lambda w, b, f: F.pack_layer(w, b, F.chain_map(32, 2), 2, f)),
    ]


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_is_bitwise_pack_layer(cuda, dtype):
    """Every case, asked for in format ``dtype`` (odd input-block counts stay fp32, as in pack_layer), in ONE launch."""
    cases = _cases(cuda)
    holder = nn.ModuleList([layer for _, layer, _ in cases])
    with pack_plan.recording() as rec:
        packed = [pack(*fused.fold_conv_bn(layer), WFMT[dtype]) for _, layer, pack in cases]
    plan = pack_plan.PackPlan(rec, holder, [])
    assert len(plan.jobs) == len(cases)
    fmts = {j.fmt for j in plan.jobs}
    assert fmts == ({fused.WFMT_F32} if dtype == "f32" else {fused.WFMT_F32, WFMT[dtype]})
    # Which cases reach the reduced formats: the kmajor and kstep_major_map cases and 16to16, 48to16 and the middle slice
    # have one or three input blocks (odd), so they are fp32 under every ``dtype``; bf16 / bf16x3 tiles come from the four
    # cases with two input blocks (32to24, pre_job_form with col0 = 3, conv_bias_no_bn, wide_running_var).  That is all
    # a single layer can show: in the network every k-step-major layer has nbi == 1 too.  Reduced-format jobs with wider
    # layers, col0 > 0 and nbi of 4 and 8 are checked by the whole-network test below, buffer by buffer.
    assert [j.nbi % 2 for j in plan.jobs].count(1) >= 5 and any(j.kmajor for j in plan.jobs)
    assert [j.fmt for j in plan.jobs].count(WFMT[dtype]) == (12 if dtype == "f32" else 4)
    want = [p.clone() for p in packed]
    for p in packed:
        p.fill_(float("nan"))                      # every element must be written, padding included
    plan.refresh()
    torch.cuda.synchronize()
    for (name, _, _), got, ref in zip(cases, packed, want):
        assert torch.equal(_bits(got), _bits(ref)), (name, dtype)
    # ... and it follows the live tensors: new values in the same storage, same plan, no new table
    table = plan._table.clone()
    with torch.no_grad():
        for _, layer, _ in cases:
            for t in list(layer.parameters()) + [b for n, b in layer.named_buffers() if "num_batches" not in n]:
                t.mul_(0.75).add_(0.01)
    plan.refresh()
    for (name, layer, pack), got in zip(cases, packed):
        assert torch.equal(_bits(got), _bits(pack(*fused.fold_conv_bn(layer), WFMT[dtype]))), (name, dtype, "edited")
    assert torch.equal(plan._table, table)


# ---- whole network -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hoist", ["1", "0"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_whole_network_refresh_equals_a_fresh_pack(cuda, monkeypatch, dtype, hoist):
    monkeypatch.setenv("PWCLO_HOIST", hoist)
    x1, x2 = _pair(cuda)                            # the pwclonet_n1024_b2 shape
    net = _net(cuda)
    net.prepare_fused(dtype=dtype)
    fs = net._fused
    assert fs.hoist == (hoist == "1")
    ptrs = {k: t.data_ptr() for k, t in fs.packed_buffers().items()}
    with torch.no_grad():
        before = fs(x1, x2).clone()
    _refill(net, "second/")
    net.refresh_fused()
    assert net._fused is fs and {k: t.data_ptr() for k, t in fs.packed_buffers().items()} == ptrs
    assert net._fused_versions == net._state_versions()
    with fused.packing_dtype(dtype):
        fresh = fused.FusedPWCLONet(net)
    _assert_buffers_equal(fs, fresh)
    with torch.no_grad():
        got, want = fs(x1, x2), fresh(x1, x2)
        assert net(x1, None, x2, None)[0].equal(want) and net._fused is fs      # the forward saw nothing to re-pack
    assert torch.equal(got, want) and not torch.equal(got, before)


# ---- graphs survive ------------------------------------------------------------------------------------------------------

def test_streaming_odometry_keeps_its_graphs(cuda):
    """Hot swap in the middle of a stream: three frames on the old weights, refresh, the fourth frame replays the SAME
    graphs and gives bit for bit what an eager fresh network with the new weights gives on the same frames (frame 3
    paired with the kept pyramid of frame 2, which the old weights produced)."""
    S = 2
    seq = torch.from_numpy(np.stack([synthetic.kitti_like_sequence(3 + i, 4096, 4)[0] for i in range(S)], axis=1)).to(cuda)
    net = _net(cuda)
    net.prepare_fused()
    so = StreamingOdometry(net, streams=S, graph=True)
    old = fused.FusedPWCLONet(net)                  # an independent packed copy of the OLD weights, run eagerly
    with torch.no_grad():
        assert so.step(seq[0]) is None
        state = old.stream_prime(seq[0], 4096)
        for k in (1, 2):
            want, state = old.stream_step(state, seq[k], 4096)
            assert torch.equal(so.step(seq[k]), want)
        entry = next(iter(so._graphs.values()))
        graph = entry["step"][0]
        _refill(net, "second/")
        net.refresh_fused()
        got = so.step(seq[3]).clone()
        fresh = fused.FusedPWCLONet(net)
        want, _ = fresh.stream_step(state, seq[3], 4096)
        stale, _ = old.stream_step(state, seq[3], 4096)
    assert len(so._graphs) == 1 and entry["step"][0] is graph and so.captures == 1
    assert torch.equal(got, want) and not torch.equal(got, stale)


def test_graphed_forward_keeps_its_graph(cuda):
    x1, x2 = _pair(cuda)
    net = _net(cuda)
    net.prepare_fused()
    gf = GraphedForward(net)
    with torch.no_grad():
        first = gf(x1, x2).clone()
        (graph, *_), = gf._graphs.values()
        _refill(net, "second/")
        net.refresh_fused()
        got = gf(x1, x2).clone()
        want = fused.FusedPWCLONet(net)(x1, x2)
    assert len(gf._graphs) == 1 and next(iter(gf._graphs.values()))[0] is graph
    assert torch.equal(got, want) and not torch.equal(got, first)


# ---- refresh inside a graph ---------------------------------------------------------------------------------------------

def test_refresh_is_capturable_and_refuses_moved_storage_under_capture(cuda):
    net = _net(cuda)
    net.prepare_fused(dtype="bf16x3")
    fs = net._fused
    fs.refresh()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fs.refresh()
    _refill(net, "second/")
    graph.replay()
    torch.cuda.synchronize()
    with fused.packing_dtype("bf16x3"):
        _assert_buffers_equal(fs, fused.FusedPWCLONet(net))
    # a swapped storage: the table would have to be written again, which a capturing stream cannot do (host-side check,
    # nothing is launched); outside capture the same call rewrites it
    p = net.psa_2.mlp_module[0].conv.weight
    p.data = p.data.clone()
    assert fs.plan.moved()
    tick = torch.zeros(1, device=cuda)
    other = torch.cuda.CUDAGraph()
    with torch.cuda.graph(other):
        tick.add_(1)
        with pytest.raises(RuntimeError, match=r"psa_2\.mlp_module\..*conv\.weight moved"):
            fs.refresh()
    fs.refresh()
    assert not fs.plan.moved()
    with fused.packing_dtype("bf16x3"):
        _assert_buffers_equal(fs, fused.FusedPWCLONet(net))
    net.refresh_fused()                             # PWCLONet level: nothing moved any more, same object
    assert net._fused is fs
    p.data = p.data.clone()
    net.refresh_fused()                             # moved, outside capture: packs again from scratch
    assert net._fused is not fs
    # The pose heads have no packed copy: they and the graphs over them read the parameters in place, so a swapped head
    # parameter cannot be refreshed by FusedPWCLONet.refresh() at all (host-side check); PWCLONet packs again.
    fs = net._fused
    q = net.pose_calculator_4.conv1d_q.conv.weight
    q.data = q.data.clone()
    with pytest.raises(RuntimeError, match=r"pose head pose_calculator_4 was swapped"):
        fs.refresh()
    net.refresh_fused()
    assert net._fused is not fs and not net._fused.plan.moved()


# ---- persistent round trip -----------------------------------------------------------------------------------------------

def test_persistent_copy_follows_training_and_load_state_dict(cuda):
    x1, x2 = _pair(cuda)
    net = _net(cuda)
    net.prepare_fused(persistent=True)
    fs = net._fused

    def check():
        with torch.no_grad():
            got = net(x1, None, x2, None)[0]
        ref = _net(cuda)
        ref.load_state_dict(net.state_dict())
        ref.eval()
        with torch.no_grad():
            want = ref(x1, None, x2, None)[0]
        assert ref._fused is not None and net._fused is fs
        assert torch.equal(got, want)
        return got.clone()

    first = check()
    net.train()
    assert net._fused is fs
    opt = torch.optim.SGD(net.parameters(), lr=1e-2)
    pose, _ = net(x1, None, x2, None)               # module path, training mode
    pose.square().sum().backward()
    opt.step()
    net.eval()
    second = check()
    assert not torch.equal(first, second)
    other = _net(cuda, fill="second/")
    net.load_state_dict(other.state_dict())
    assert net._fused is fs
    third = check()
    assert not torch.equal(second, third)
