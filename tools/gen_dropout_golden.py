"""Golden values of ONE training step of the imported reference with DROPOUT ON, under the masks of
``training.DropoutStream`` -- test infrastructure, for the container that holds the reference tree.

    python tools/gen_dropout_golden.py        (writes tests/golden/train_dropout_n1024_b2.npz and ..._b2_grad64.npz)

The counterpart of ``oracle/gen_train_golden.py`` (whose helpers it imports) for the mode that file switches off: the
reference model stays FULLY in ``train()``, and while its forward runs ``torch.nn.functional.dropout`` is replaced by a
function that multiplies its input by ``2 * mask[call // 2, call % 2]`` -- the keep masks of tests/dropout_model.py at
(SEED, STEP, RANK), DESIGN.md section 15.  The reference's four heads call dropout twice each, first for the q branch
and then for the t branch (PW/pose_calculator.py:63-65), in the order pose_calculator_4, pose_warp_refinement_3, _2, _1:
exactly 8 calls with p = 0.5, which is asserted.  The reference's random stream is not reproduced; its law is.

Recorded: everything ``train_n1024_b2.npz`` holds (fp32 and float64 reference steps), plus ``masks`` (4,2,B,256) bool and
seed / step / rank in ``meta``; the 17 float64 gradients (``grad64.*``) go into the second file so that each stays below
the 1 MiB limit for a committed file.  Nothing is written into oracle/.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle import gen_golden, ops, params, ref_import                      # noqa: E402
from oracle.gen_grad_golden import ground_truth                              # noqa: E402
from oracle.gen_train_golden import BN_LAYERS, TRAIN_PARAMS, _install_float64_ext   # noqa: E402
import dropout_model                                                         # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "train_dropout_n1024_b2.npz")
OUT64 = os.path.join(ROOT, "tests", "golden", "train_dropout_n1024_b2_grad64.npz")
CASE = "n1024_b2"
SEED, STEP, RANK = (1 << 63) + 20240, 1, 1       # a seed with the high word set, a non-zero step and rank


class MaskedDropout:
    """Stands in for ``torch.nn.functional.dropout`` during one forward."""

    def __init__(self, masks):
        self.masks, self.calls = masks, 0

    def __call__(self, x, p=0.5, training=True, inplace=False):
        assert p == 0.5 and training and not inplace, (p, training, inplace)
        assert self.calls < 8, "more than 8 dropout calls in one forward"
        m = self.masks[self.calls // 2, self.calls % 2]
        self.calls += 1
        assert x.shape == m.shape + (1,), (x.shape, m.shape)
        return x * (2.0 * torch.from_numpy(m.astype(np.float64)).to(x.dtype).unsqueeze(2))


def masked_step(model, loss_mod, x1, x2, gt, masks):
    """forward + loss + backward of a reference model in train() with ``F.dropout`` replaced for the forward."""
    import torch.nn.functional as F
    model.train()
    assert all(m.training for m in model.modules())
    stand_in, real = MaskedDropout(masks), F.dropout
    F.dropout = stand_in
    try:
        pose, _ = model(x1, None, x2, None)
    finally:
        F.dropout = real
    assert stand_in.calls == 8, stand_in.calls
    loss, _ = loss_mod(pose, gt)
    loss.backward()
    return pose.detach(), loss.detach()


def main():
    ns = ref_import.load()
    lm = ref_import.load_loss()
    x1, x2 = gen_golden.case_inputs(CASE)
    B = x1.shape[0]
    masks = dropout_model.keep_masks(SEED, STEP, RANK, B)
    cfg = ns.DictConfig(mode="supervised", loss_degrees=False, loss_weights=[1.0, 1.0], with_exp_weights=True,
                        init_weights=[0.0, -2.5], loss_option="l2_norm", nb_levels=4, device="cpu", scalar_last=False)
    ref_knn = ns.pytorch_utils.knn_point
    ns.pytorch_utils.knn_point = lambda k, xyz, new_xyz: ops.knn_point(k, xyz.float().contiguous(),
                                                                        new_xyz.float().contiguous())
    try:
        model = ref_import.make_reference_model()
        params.fill_state_dict(model.state_dict())
        loss_mod = lm._PWCLONetLossModule(cfg, lm.Pose("quaternions"))
        pose, loss = masked_step(model, loss_mod, x1, x2, ground_truth(B), masks)
        _install_float64_ext(ns)
        model64 = ref_import.make_reference_model()
        params.fill_state_dict(model64.state_dict())
        model64 = model64.double()
        loss_mod64 = lm._PWCLONetLossModule(cfg, lm.Pose("quaternions")).double()
        pose64, loss64 = masked_step(model64, loss_mod64, x1.double(), x2.double(), ground_truth(B).double(), masks)
    finally:
        ns.pytorch_utils.knn_point = ref_knn
    named, named64 = dict(model.named_parameters()), dict(model64.named_parameters())
    missing = [k for k, p in named.items() if p.grad is None]
    assert not missing, missing
    sd = model.state_dict()
    out = {"loss": loss.numpy(), "pose_params": pose.numpy(), "grad_s": loss_mod.exp_weighting.s_param.grad.numpy(),
           "loss64": loss64.numpy(), "pose64": pose64.numpy(), "grad64_s": loss_mod64.exp_weighting.s_param.grad.numpy(),
           "masks": masks}
    for k in TRAIN_PARAMS:
        out["grad." + k] = named[k].grad.numpy()
        out["grad64." + k] = named64[k].grad.numpy()
        e = (named[k].grad.double() - named64[k].grad).abs().max().item() / named64[k].grad.abs().max().item()
        print("%-78s |g|max %.3e   fp32 reference vs float64 reference: %.2e of max|g|"
              % (k, named[k].grad.abs().max().item(), e))
    for k in BN_LAYERS:
        for s in ("running_mean", "running_var", "num_batches_tracked"):
            out["buf.%s.%s" % (k, s)] = sd["%s.%s" % (k, s)].numpy()
    names = sorted(named)
    out["all_grad_absmax"] = np.array([named[k].grad.abs().max().item() for k in names], dtype=np.float64)
    out["all_grad_l2"] = np.array([named[k].grad.double().norm().item() for k in names], dtype=np.float64)
    out["all_grad64_absmax"] = np.array([named64[k].grad.abs().max().item() for k in names], dtype=np.float64)
    out["all_grad64_l2"] = np.array([named64[k].grad.norm().item() for k in names], dtype=np.float64)
    out["all_ref32_err"] = np.array([(named[k].grad.double() - named64[k].grad).abs().max().item()
                                     / max(named64[k].grad.abs().max().item(), 1e-300) for k in names])
    # The GPU test judges every tensor in units of max|g64|.  That unit is meaningless for a tensor whose true gradient is
    # the residue of a cancellation: at steps 2, 7 and 8 the finest head's t bias received +c and -c from the two clouds -- exactly 0
    # in the fp32 reference, 3e-12 in float64, "error" 1.0 -- and one ulp of c is a thousand units.  Such a step is no
    # fixture: take another one.
    assert out["all_ref32_err"].max() < 0.1, [(k, e) for k, e in zip(names, out["all_ref32_err"]) if e >= 0.1]
    # The GPU test also holds the pose to 1e-5 of the fp32 values.  Where the reference's own fp32 pose is further than a
    # quarter of that from its float64 pose (steps 3 and 6: 8.9e-6 and 1.1e-5 of the scale; the finest level's neighbour
    # lists sit on near-ties there), two fp32 implementations cannot be expected inside it, and a flipped neighbour moves
    # gradients by 1e-2: no fixture either.
    pose_err = float(np.abs(out["pose_params"].astype(np.float64) - out["pose64"]).max() / np.abs(out["pose64"]).max())
    print("fp32 reference vs float64 reference, pose: %.2e of the scale" % pose_err)
    assert pose_err <= 2.5e-6, pose_err
    out["meta"] = np.array(json.dumps(dict(
        case=CASE, params=TRAIN_PARAMS, bn_layers=BN_LAYERS, gt_seed=515, all_names=names, seed=SEED, step=STEP, rank=RANK,
        mode="train (batch-statistic BN), dropout ON under the DropoutStream masks (F.dropout replaced for the forward)",
        knn="oracle (IEEE key, ties -> lower index)")))
    # two files, each below the repository's 1 MiB limit for a committed file: the float64 gradients travel apart
    wide = {k: out.pop(k) for k in [k for k in out if k.startswith("grad64.")]}
    np.savez_compressed(OUT, **out)
    np.savez_compressed(OUT64, **wide)
    for f in (OUT, OUT64):
        assert os.path.getsize(f) < (1 << 20), (f, os.path.getsize(f))
        print("wrote", f, os.path.getsize(f), "bytes")
    print("loss", float(loss))


if __name__ == "__main__":
    main()
