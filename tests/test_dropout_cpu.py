"""Dropout-on training, the parts that need no GPU: the mask law of tests/dropout_model.py, the
masked restatement of the CPU oracle pinned to values recorded from the imported reference with dropout ON
(tests/golden/train_dropout_n1024_b2*.npz, tools/gen_dropout_golden.py), and ``training.DropoutStream``'s argument checks.
"""
import json
import os

import numpy as np
import pytest
import torch

import dropout_model as DM
from oracle import gen_golden, params
from oracle import model as M
from oracle.gen_grad_golden import ground_truth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_fixture():
    """Both files of the fixture as one dict (the float64 gradients are kept apart for the file-size limit)."""
    z = dict(np.load(os.path.join(GOLDEN, "train_dropout_n1024_b2.npz")))
    z.update(np.load(os.path.join(GOLDEN, "train_dropout_n1024_b2_grad64.npz")))
    return z, json.loads(str(z["meta"]))


def fresh_state_dict():
    with open(os.path.join(GOLDEN, "state_shapes.json")) as f:
        return params.make_state_dict(json.load(f))


def test_mask_law():
    """Fair bits (n independent bits: sigma = 0.5 / sqrt(n), every bound is 4 sigma), the step enters modulo 2^32, rank,
    head and branch select independent words, the seed's high word is part of the key."""
    m = DM.keep_masks(0, 0, 0, 32)
    assert m.shape == (4, 2, 32, 256) and m.dtype == np.bool_
    sigma = 0.5 / np.sqrt(m.size)
    assert abs(sigma - 0.00195) < 1e-5
    print("\nkeep fraction %.4f (%.1f sigma)" % (m.mean(), (m.mean() - 0.5) / sigma))
    assert abs(m.mean() - 0.5) <= 4 * sigma
    assert np.array_equal(DM.keep_masks(0, 1, 0, 32), DM.keep_masks(0, (1 << 32) + 1, 0, 32))
    assert not np.array_equal(DM.keep_masks(0, 1, 0, 32), DM.keep_masks(0, 2, 0, 32))
    other = (m != DM.keep_masks(0, 0, 1, 32)).mean()
    print("ranks 0 and 1 differ in %.4f of the bits" % other)
    assert abs(other - 0.5) <= 4 * sigma
    sigma_head = 0.5 / np.sqrt(32 * 256)
    for h in range(4):
        agree = (m[h, 0] == m[h, 1]).mean()
        print("head %d: q and t masks agree in %.4f of the units" % (h, agree))
        assert abs(agree - 0.5) <= 4 * sigma_head
        for g in range(h):
            assert abs((m[h] == m[g]).mean() - 0.5) <= 4 * sigma_head
    # clouds of a larger batch keep their masks: the counter holds the cloud, not the batch size
    assert np.array_equal(DM.keep_masks(0, 0, 0, 2), m[:, :, :2])
    high = (1 << 63) + 5
    mh = DM.keep_masks(high, 3, 2, 32)
    assert abs(mh.mean() - 0.5) <= 4 * sigma
    assert abs((mh != DM.keep_masks(5, 3, 2, 32)).mean() - 0.5) <= 4 * sigma             # the high word matters
    assert np.array_equal(mh, DM.keep_masks(high - (1 << 64), 3, 2, 32))                 # the same 64 bits, signed
    # the non-vacuity figures of the B = 1 exact-zero test
    assert [int((~DM.keep_masks(2024, 0, 0, 1)[h, 0]).sum()) for h in range(4)] == [131, 146, 121, 131]


def test_patched_oracle_with_all_keep_masks_is_the_oracle(monkeypatch):
    """The patch itself changes nothing: all-keep masks at scale 1 give the unpatched step bit for bit."""
    x1, x2 = gen_golden.case_inputs("n1024_b2")
    gt = ground_truth(2)
    plain = M.pwclonet_train_step(fresh_state_dict(), x1, x2, gt)
    head = DM.masked_pose_calculator(np.ones((4, 2, 2, 256), dtype=bool), scale=1.0)
    monkeypatch.setattr(M, "pose_calculator", head)
    patched = M.pwclonet_train_step(fresh_state_dict(), x1, x2, gt)
    assert head.state["calls"] == 4
    assert torch.equal(plain[0], patched[0]) and torch.equal(plain[1], patched[1]) and torch.equal(plain[3], patched[3])
    assert plain[2].keys() == patched[2].keys()
    for k, g in plain[2].items():
        assert torch.equal(g, patched[2][k]), k


def test_masked_oracle_matches_reference_dropout_golden(monkeypatch):
    """``oracle.model.pwclonet_train_step`` with ``masked_pose_calculator(fixture masks)`` against the values recorded
    from the imported reference, fully in train() with F.dropout replaced by the same masks: the bounds
    tests/test_oracle_cpu.py applies to train_n1024_b2.npz, in fp32 and in float64."""
    z, meta = load_fixture()
    masks = z["masks"]
    assert np.array_equal(masks, DM.keep_masks(meta["seed"], meta["step"], meta["rank"], masks.shape[2]))
    x1, x2 = gen_golden.case_inputs(meta["case"])
    gt = ground_truth(x1.shape[0])
    monkeypatch.setattr(M, "pose_calculator", DM.masked_pose_calculator(masks))
    sd = fresh_state_dict()
    pose, loss, grads, gs = M.pwclonet_train_step(sd, x1, x2, gt)
    np.testing.assert_allclose(pose.numpy(), z["pose_params"], rtol=0, atol=2e-6)
    assert abs(loss.item() - float(z["loss"])) <= 1e-6 * abs(float(z["loss"]))
    for k in meta["params"]:
        ref = z["grad." + k]
        err = np.abs(grads[k].numpy() - ref).max() / np.abs(ref).max()
        print("%-78s fp32 %.2e" % (k, err))
        assert err <= 5e-5, k
    np.testing.assert_allclose(gs.numpy(), z["grad_s"], rtol=1e-6)
    for k in meta["bn_layers"]:
        np.testing.assert_allclose(sd[k + ".running_mean"].numpy(), z["buf.%s.running_mean" % k], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(sd[k + ".running_var"].numpy(), z["buf.%s.running_var" % k], rtol=1e-6, atol=1e-7)
        assert int(sd[k + ".num_batches_tracked"]) == int(z["buf.%s.num_batches_tracked" % k])
    l2 = np.array([grads[k].double().norm().item() for k in meta["all_names"]])
    np.testing.assert_allclose(l2, z["all_grad_l2"], rtol=1e-4, atol=1e-7 * z["all_grad_l2"].max())
    # dropout changed the step: this is not the dropout-off fixture again
    off = np.load(os.path.join(GOLDEN, "train_n1024_b2.npz"))
    assert abs(float(off["loss"]) - float(z["loss"])) > 1e-3 * abs(float(z["loss"]))
    pose, loss, grads, gs = M.pwclonet_train_step(fresh_state_dict(), x1, x2, gt, dtype=torch.float64)
    np.testing.assert_allclose(pose.numpy(), z["pose64"], rtol=0, atol=1e-12)
    assert abs(loss.item() - float(z["loss64"])) <= 1e-12 * abs(float(z["loss64"]))
    for k in meta["params"]:
        ref = z["grad64." + k]
        assert np.abs(grads[k].numpy() - ref).max() <= 1e-10 * np.abs(ref).max(), k
    l2 = np.array([grads[k].norm().item() for k in meta["all_names"]])
    np.testing.assert_allclose(l2, z["all_grad64_l2"], rtol=1e-10)


class _Head(torch.nn.Module):
    def from_logits(self, emb, logits):
        raise AssertionError("not called")


class _Net(torch.nn.Module):
    """The four head slots of PWCLONet, nothing else: attaching needs no weights and no GPU."""

    def __init__(self):
        super().__init__()
        self.pose_calculator_4 = _Head()
        for k in (3, 2, 1):
            holder = torch.nn.Module()
            holder.pose_calculator = _Head()
            setattr(self, "pose_warp_refinement_%d" % k, holder)


def test_dropout_stream_argument_validation():
    from pwclonet_pylidarslam_amd.training import DropoutStream
    for bad in (1 << 64, -(1 << 63) - 1):
        with pytest.raises(ValueError):
            DropoutStream(_Net(), seed=bad)
    for bad in (-1, 1 << 28):
        with pytest.raises(ValueError):
            DropoutStream(_Net(), rank=bad)
    with pytest.raises(TypeError):
        DropoutStream(torch.nn.Linear(2, 2))
    with pytest.raises(TypeError):
        DropoutStream(object())
    net = _Net()
    ds = DropoutStream(net, seed=-1, rank=(1 << 28) - 1)
    assert ds.seed == (1 << 64) - 1 and ds.rank == (1 << 28) - 1
    assert net._dropout_stream is ds
    assert [net.get_submodule(n)._dropout_stream for n in DropoutStream.HEADS] == [(ds, 0), (ds, 1), (ds, 2), (ds, 3)]
    with pytest.raises(RuntimeError):
        DropoutStream(net)                                   # one stream per network
    assert ds.step_index() == 0
    ds.set_step(41)
    assert ds.step_index() == 41
    ds.set_step((1 << 62) - 1)
    for bad in (-1, 1 << 62):
        with pytest.raises(ValueError):
            ds.set_step(bad)
    with pytest.raises(RuntimeError):
        ds.masks()                                           # nothing has run
    sd = ds.state_dict()
    assert sd == {"seed": (1 << 64) - 1, "rank": (1 << 28) - 1, "step": (1 << 62) - 1}
    ds.detach()
    assert net._dropout_stream is None and net.pose_calculator_4._dropout_stream is None
    other = DropoutStream(net, seed=3)
    other.load_state_dict(sd)
    assert other.state_dict() == sd
    for bad in ({"seed": 1 << 64, "rank": 0, "step": 0}, {"seed": 0, "rank": 1 << 28, "step": 0},
                {"seed": 0, "rank": 0, "step": -1}):
        with pytest.raises(ValueError):
            other.load_state_dict(bad)
