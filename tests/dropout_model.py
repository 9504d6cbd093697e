"""Host model of ``training.DropoutStream``'s mask law and the masked pose head of the CPU oracle (a test helper: not a
conftest, not a product module).

Written from the rules of DESIGN.md section 15, not from the kernels:

* keep bit of hidden unit ``c`` of cloud ``b`` in head ``h`` (0 = pose_calculator_4, 1..3 = pose_warp_refinement_3, _2, _1:
  forward order), branch 0 = q / 1 = t: the top bit of output word 0 of Philox4x32-10 under key (seed low word, seed high
  word) at counter ``(b * 256 + c, rank * 8 + h * 2 + branch, step mod 2^32, 3)``;
* a kept value is multiplied by 2, a dropped one is 0 (``F.dropout`` at p = 0.5).
"""
import numpy as np
import torch
import torch.nn.functional as F

from train_batch_model import philox4x32_10

DROPOUT = 3          # purpose word; 0, 1, 2 belong to the batch builder
HIDDEN = 256


def keep_masks(seed, step, rank, B):
    """-> (4, 2, B, 256) bool: [head, branch, cloud, unit]."""
    seed = int(seed) & ((1 << 64) - 1)
    index = (np.arange(B, dtype=np.uint64)[:, None] * np.uint64(HIDDEN) + np.arange(HIDDEN, dtype=np.uint64)[None, :])
    out = np.zeros((4, 2, B, HIDDEN), dtype=bool)
    for head in range(4):
        for branch in range(2):
            unit = int(rank) * 8 + head * 2 + branch
            word = philox4x32_10((index, unit, int(step) & 0xFFFFFFFF, DROPOUT), (seed & 0xFFFFFFFF, seed >> 32))[0]
            out[head, branch] = (word >> np.uint32(31)) != 0
    return out


def masked_pose_calculator(masks, scale=2.0):
    """A function with the signature of ``oracle.model.pose_calculator`` whose n-th call (n = 0..3, then again from 0)
    multiplies the hidden vector by ``scale * masks[n, 0]`` on the q branch and ``scale * masks[n, 1]`` on the t branch."""
    masks = np.asarray(masks)
    assert masks.shape[:2] == (4, 2) and masks.shape[3] == HIDDEN, masks.shape
    state = {"calls": 0}

    def pose_calculator(sd, prefix, emb, mask):
        m = masks[state["calls"] % 4]
        state["calls"] += 1
        s = torch.sum(emb * mask, dim=2, keepdim=True)
        big = F.conv1d(s, sd[prefix + ".conv1d_q_t.conv.weight"], sd[prefix + ".conv1d_q_t.conv.bias"])
        mq = torch.from_numpy(m[0].astype(np.float64)).to(big.dtype).unsqueeze(2) * scale
        mt = torch.from_numpy(m[1].astype(np.float64)).to(big.dtype).unsqueeze(2) * scale
        q = F.conv1d(big * mq, sd[prefix + ".conv1d_q.conv.weight"], sd[prefix + ".conv1d_q.conv.bias"])
        q = q / (torch.sqrt(torch.sum(q * q, dim=1, keepdim=True) + 1e-10) + 1e-10)
        t = F.conv1d(big * mt, sd[prefix + ".conv1d_t.conv.weight"], sd[prefix + ".conv1d_t.conv.bias"])
        return q, t

    pose_calculator.state = state
    return pose_calculator
