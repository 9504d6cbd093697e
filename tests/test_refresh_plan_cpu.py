"""The pack plan (pwclonet_pylidarslam_amd/pack_plan.py) on the CPU: a NumPy restatement of the index map of
csrc/pack_refresh.hip, written here from the documented tile layouts (fused.pack_layer, csrc/mlp_core.hpp), executes the
plan a ``FusedPWCLONet`` recorded while packing and must reproduce every packed buffer bit for bit, writing every
element exactly once -- for fp32 / bf16x3 / bf16 packing and for the hoisted and the section-3 class families."""
import numpy as np
import pytest
import torch

from oracle import params
from pwclonet_pylidarslam_amd import fused, pack_plan
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet


def _net():
    net = PWCLONet(dict(num_input_channels=3, sequence_len=2, device="cpu", scalar_last=False, log_mode="none"))
    params.fill_state_dict(net.state_dict())
    return net.eval()


# ---- the kernel's arithmetic and index map, restated -------------------------------------------------------------------

def _bf16_bits(x):
    """float32 array -> bf16 bit patterns (uint32 holding 16 bits), round to nearest even."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return (u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)


def _bf16_value(bits):
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)


def _folded(job):
    """fold_conv_bn's arithmetic on the job's live tensors: (W' (cout, cin), b' (cout,)) float32."""
    t = job.tensors()
    f64 = lambda x: x.detach().numpy().astype(np.float64)
    w = f64(t["w"]).reshape(job.cout, job.cin)
    b = f64(t["conv_bias"]) if t["conv_bias"] is not None else np.zeros(job.cout)
    if t["var"] is not None:
        s = f64(t["gamma"]) / np.sqrt(f64(t["var"]) + t["eps"])
        w = w * s[:, None]
        b = (b - f64(t["mean"])) * s + f64(t["beta"])
    return w.astype(np.float32), b.astype(np.float32)


def _run_job(job, halves, counts):
    """Execute one job the way the kernel's threads do: per destination element its (output row, physical input channel),
    the value, and the destination offset.  ``halves``: the destination buffer as uint16 halves (two per float);
    ``counts``: writes per half."""
    w, b = _folded(job)
    pm = np.asarray(job.phys_map)
    nbo, nbi = job.nbo, job.nbi

    def channel(prow):                         # output channel on physical row prow, -1 = padding
        c = np.where(job.kmajor, 4 * (prow % 4) + prow // 4, prow)
        return np.where(c < job.cout, c, -1)

    def weight(prow, pch):                     # broadcasts
        c, col = channel(prow), pm[pch]
        ok = (c >= 0) & (col >= 0)
        return np.where(ok, w[np.where(ok, c, 0), np.where(ok, job.col0 + col, 0)], np.float32(0)).astype(np.float32)

    def store32(off, bits):                    # fp32 words at float offsets `off` of the job
        lo = 2 * (job.dst_off + off.ravel())
        for k in (0, 1):
            halves[lo + k] = ((bits.ravel() >> np.uint32(16 * k)) & np.uint32(0xffff)).astype(np.uint16)
            np.add.at(counts, lo + k, 1)

    def store16(off_halves, bits):             # bf16 values at half offsets of the job
        at = 2 * job.dst_off + off_halves.ravel()
        halves[at] = bits.ravel().astype(np.uint16)
        np.add.at(counts, at, 1)

    lane = np.arange(64)
    row, g = lane % 16, lane // 16
    if job.fmt == fused.WFMT_F32:              # [o][m][lane][4]: element r = physical channel 16 m + 4 g + r
        o, m, ln, r = np.meshgrid(np.arange(nbo), np.arange(nbi), lane, np.arange(4), indexing="ij")
        val = weight(16 * o + row[ln], 16 * m + 4 * g[ln] + r)
        store32(((o * nbi + m) * 64 + ln) * 4 + r, val.view(np.uint32))
        tile_floats = nbo * nbi * 256
    else:                                      # [o][mp]([split])[lane][8]: element e = channel 16 (2 mp + e // 4) + 4 g + e % 4
        nsplit = 3 if job.fmt == fused.WFMT_BF16X3 else 1
        o, mp, ln, e = np.meshgrid(np.arange(nbo), np.arange(nbi // 2), lane, np.arange(8), indexing="ij")
        val = weight(16 * o + row[ln], 16 * (2 * mp + e // 4) + 4 * g[ln] + e % 4)
        hi = _bf16_bits(val)
        r1 = (val - _bf16_value(hi)).astype(np.float32)
        mid = _bf16_bits(r1)
        lo = _bf16_bits((r1 - _bf16_value(mid)).astype(np.float32))
        for split, bits in enumerate((hi, mid, lo)[:nsplit]):
            store16((((o * (nbi // 2) + mp) * nsplit + split) * 64 + ln) * 8 + e, bits)
        tile_floats = nbo * (nbi // 2) * nsplit * 256
    prow = np.arange(16 * nbo)
    c = channel(prow)
    bias = np.where((c >= 0) & job.use_bias, b[np.where(c >= 0, c, 0)], np.float32(0)).astype(np.float32)
    store32(tile_floats + prow, bias.view(np.uint32))
    assert tile_floats + 16 * nbo == job.floats


def _execute(plan, buffers):
    """Run every job of ``plan`` into zero-initialised copies of ``buffers`` ({name: tensor}) -> ({name: uint16 halves},
    {name: write counts})."""
    by_ptr = {t.data_ptr(): name for name, t in buffers.items()}
    assert len(by_ptr) == len(buffers)
    out = {name: np.zeros(2 * t.numel(), dtype=np.uint16) for name, t in buffers.items()}
    counts = {name: np.zeros(2 * t.numel(), dtype=np.int64) for name, t in buffers.items()}
    for job in plan.jobs:
        name = by_ptr[job.dst.data_ptr()]      # KeyError: a job writes somewhere the kernels never read
        _run_job(job, out[name], counts[name])
    return out, counts


@pytest.mark.parametrize("hoist", ["1", "0"])
@pytest.mark.parametrize("dtype", ["f32", "bf16x3", "bf16"])
def test_plan_reproduces_every_packed_buffer(monkeypatch, dtype, hoist):
    monkeypatch.setenv("PWCLO_HOIST", hoist)
    net = _net()
    with fused.packing_dtype(dtype):
        fs = fused.FusedPWCLONet(net)
    assert fs.hoist == (hoist == "1")
    buffers = fs.packed_buffers()
    # the figures DESIGN.md section 16 quotes: one job per pack_layer call, one buffer per tensor the kernels read
    assert (len(fs.plan.jobs), len(buffers)) == ((107, 61) if hoist == "1" else (81, 35))
    if dtype != "f32":
        # (the section-3 classes have no bf16 stacks: fused.cv_stack_wfmt)
        assert any(j.fmt == fused._DTYPE_WFMT[dtype] for j in fs.plan.jobs) == ((dtype, hoist) != ("bf16", "0"))
        assert any(j.fmt == fused.WFMT_F32 for j in fs.plan.jobs)          # odd layers stay fp32
    got, counts = _execute(fs.plan, buffers)
    written = 0
    for name, t in buffers.items():
        want = t.contiguous().view(torch.int16).numpy().view(np.uint16)
        assert (counts[name] == 1).all(), "%s: %d elements not written exactly once" % (name, (counts[name] != 1).sum())
        assert np.array_equal(got[name], want), name
        written += counts[name].sum()
    assert written == 2 * sum(t.numel() for t in buffers.values()) == 2 * sum(j.floats for j in fs.plan.jobs)
    assert fs.plan.total_tiles == sum(j.tiles for j in fs.plan.jobs)
    assert all(j.name != "?" for j in fs.plan.jobs)


def test_plan_covers_the_kmajor_forms(monkeypatch):
    """PWCLO_SA_KMAJOR: level 0's k-step-major layers are jobs with ``kmajor`` when on, plain jobs when off; both plans
    reproduce their buffers (the default-on form is part of the test above as well)."""
    for flag, want in (("1", 2), ("0", 0)):
        monkeypatch.setenv("PWCLO_SA_KMAJOR", flag)
        fs = fused.FusedPWCLONet(_net())
        assert fs.sa[0].kmajor == int(flag)
        assert sum(j.kmajor for j in fs.plan.jobs) == want
        buffers = {"sa1.packed": fs.sa[0].packed}
        plan = type("P", (), {"jobs": [j for j in fs.plan.jobs if j.dst.data_ptr() == fs.sa[0].packed.data_ptr()]})
        got, counts = _execute(plan, buffers)
        assert (counts["sa1.packed"] == 1).all()
        assert np.array_equal(got["sa1.packed"], fs.sa[0].packed.view(torch.int16).numpy().view(np.uint16))


def test_plan_follows_the_live_tensors():
    """The jobs read the module at execution time: after an in-place edit of every parameter and buffer the same plan
    reproduces a FRESH pack, not the old one."""
    net = _net()
    fs = fused.FusedPWCLONet(net)
    with torch.no_grad():
        for k, v in net.state_dict().items():
            v.copy_(torch.from_numpy(np.array(params.fill_value("second/" + k, v.shape))).reshape(v.shape).to(v.dtype))
    fresh = fused.FusedPWCLONet(net).packed_buffers()
    got, _ = _execute(fs.plan, fs.packed_buffers())
    changed = 0
    for name, t in fresh.items():
        assert np.array_equal(got[name], t.view(torch.int16).numpy().view(np.uint16)), name
        changed += int(not torch.equal(t, fs.packed_buffers()[name]))
    assert changed == len(fresh)


def test_pose_head_weights_alias_the_parameters():
    net = _net()
    fs = fused.FusedPWCLONet(net)
    assert len(fs.plan.heads) == 4
    for head, module, _ in fs.plan.heads:
        assert pack_plan.head_aliases(head, module)
        assert head.w_qt.shape == (256, 64) and head.w_qt.is_contiguous()
    names = [n for n, _ in fs.plan.sources()]
    assert len(names) == len(set(names)) and "pose_calculator_4.conv1d_q.conv.bias" in names
    assert not fs.plan.moved()                    # no device table on the CPU: nothing to compare against


def test_refresh_failure_paths_and_persistence():
    net = _net()
    with pytest.raises(RuntimeError, match="not packed"):
        net.refresh_fused()
    net.prepare_fused()                           # default: today's behaviour
    assert net._fused is not None
    net.train()
    assert net._fused is None
    net.prepare_fused()
    net.load_state_dict(net.state_dict())
    assert net._fused is None
    net.prepare_fused(persistent=True)
    fs = net._fused
    net.train()
    net.eval()
    net.load_state_dict(net.state_dict())
    assert net._fused is fs
    with pytest.raises(RuntimeError, match="CPU not supported"):      # the refresh itself is a GPU launch, no fallback
        net.refresh_fused()
    sd = net.state_dict()
    net.load_state_dict(sd, True, True)           # assign=True, given by position: the parameters themselves are swapped
    assert net._fused is None
    net.prepare_fused(persistent=True)
    net.load_state_dict(sd, True, False)
    assert net._fused is not None
    net.train()
    with pytest.raises(RuntimeError, match="CPU not supported"):
        net.refresh_fused()
    assert not net.training                       # documented: refresh_fused puts the module into eval mode
    net.float()                                   # _apply: the storage may move
    assert net._fused is None
    net.prepare_fused()                           # an explicit default call ends persistence
    net.train()
    assert net._fused is None
