"""CPU tests (``-m "not gpu"``) of the flat data-parallel step's host logic (pwclonet_pylidarslam_amd/flat_step.py):
the bucket layout, the 2-rank (gloo) all-reduce of pre-scaled buckets with their non-finite count slot, and what the
classes refuse.  The kernels are tested on the GPU (tests/test_gpu_flat_step.py)."""
import ast
import os
import subprocess
import sys

import pytest
import torch

from pwclonet_pylidarslam_amd import flat_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bucket_layout_by_hand():
    offsets, total = flat_step.bucket_layout([1, 2, 3, 64, 65])
    assert offsets == [0, 64, 128, 192, 256]
    assert total == 256 + 128 + 1                      # the last tensor ends at 321 -> 384, plus the count slot
    assert flat_step.bucket_layout([]) == ([], 1)
    assert flat_step.bucket_layout([0, 5]) == ([0, 0], 65)
    assert flat_step.bucket_layout([3, 3], align_values=4) == ([0, 4], 9)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_bucket_layout_aligned_and_disjoint(seed):
    g = torch.Generator().manual_seed(seed)
    sizes = [int(s) for s in torch.randint(1, 5000, (200,), generator=g)] + [1, 63, 64, 65, 128]
    offsets, total = flat_step.bucket_layout(sizes)
    assert len(offsets) == len(sizes) and offsets[0] == 0
    assert all(o % 64 == 0 for o in offsets)                                           # 256-byte aligned
    assert all(o + s <= nxt for o, s, nxt in zip(offsets, sizes, offsets[1:]))         # no overlap, in order
    assert all(nxt - (o + s) < 64 for o, s, nxt in zip(offsets, sizes, offsets[1:]))   # less than one unit of padding
    last_end = offsets[-1] + sizes[-1]
    assert total == (last_end + 63) // 64 * 64 + 1


def test_bucket_layout_of_the_training_unit():
    from pwclonet_pylidarslam_amd.loss import PWCLONetLossModule
    from pwclonet_pylidarslam_amd.pwclonet import PWCLONet
    from pwclonet_pylidarslam_amd.training import FlatAdam, FlatTrainStep, PWCLONetWithLoss
    assert FlatAdam is flat_step.FlatAdam and FlatTrainStep is flat_step.FlatTrainStep      # exported from training.py
    net = PWCLONet(dict(num_input_channels=3, sequence_len=2, device="cpu", scalar_last=False))
    unit = PWCLONetWithLoss(net, PWCLONetLossModule(dict(with_exp_weights=True, init_weights=[0.0, -2.5],
                                                         loss_option="l2_norm", nb_levels=4, scalar_last=False)))
    sizes = [p.numel() for p in unit.parameters() if p.requires_grad]
    assert sum(sizes) == 775070 and sizes[-1] == 2          # the loss module's s_param pair travels in the bucket
    offsets, total = flat_step.bucket_layout(sizes)
    assert total >= 775070 + 1 and total - 1 - 775070 < 64 * len(sizes)
    with pytest.raises(RuntimeError, match="CPU not supported"):       # no CPU path
        FlatAdam(unit.parameters(), lr=1e-3)


def test_other_optimizers_are_refused():
    assert flat_step.refuse_other_optimizers("adam") is False
    assert flat_step.refuse_other_optimizers("adamw") is True
    for kind in ("sgd", "rmsprop"):
        with pytest.raises(NotImplementedError, match="'adam' and 'adamw' only"):
            flat_step.refuse_other_optimizers(kind)
    with pytest.raises(TypeError, match="FlatAdam"):
        flat_step.FlatTrainStep(torch.nn.Linear(2, 2), torch.optim.Adam([torch.zeros(2, requires_grad=True)]), None, None,
                                None)


WORKER = r"""
import os, sys, torch
sys.path.insert(0, %r)
import torch.distributed as dist
from pwclonet_pylidarslam_amd import dist_util, flat_step
rank, world = dist_util.init("gloo")
sizes = [1, 2, 3, 64, 65]
offsets, total = flat_step.bucket_layout(sizes)
g = torch.Generator().manual_seed(10 + rank)               # different gradients per rank
local = torch.zeros(total)
for o, s in zip(offsets, sizes):
    local[o:o + s] = torch.randn(s, generator=g)
bucket = local / world                                      # what pack(1 / world) leaves: pre-scaled values ...
bucket[total - 1] = float(rank + 1)                         # ... and this rank's own count of non-finite values
both = [torch.zeros(total) for _ in range(world)]
dist.all_gather(both, local)
dist.all_reduce(bucket, op=dist.ReduceOp.SUM)
mean = sum(b.double() for b in both) / world
err = (bucket[:total - 1].double() - mean[:total - 1]).abs().max().item()
pad = torch.ones(total, dtype=torch.bool)
pad[total - 1] = False
for o, s in zip(offsets, sizes):
    pad[o:o + s] = False
print("RESULT", rank, [err, float(bucket[total - 1]), float(bucket[pad].abs().max())], bucket[:4].tolist(),
      [float(bucket.double().sum())], flush=True)
dist_util.finish()
"""


def test_two_rank_gloo_bucket_all_reduce(tmp_path):
    """2 ranks, gloo, CPU tensors, no kernel: after ``all_reduce(SUM)`` of the pre-scaled buckets both ranks hold the
    same bucket, equal to the mean of the ranks' gradients; the padding stays zero and the count slot holds the SUM of
    the ranks' counts (1 + 2), so every rank reaches the same skip verdict."""
    script = tmp_path / "flat_worker.py"
    script.write_text(WORKER % ROOT)
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2",
                   MASTER_ADDR="127.0.0.1", MASTER_PORT="29623")
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=180)[0] for p in procs]
    rows = sorted(l for o in outs for l in o.splitlines() if l.startswith("RESULT"))
    assert len(rows) == 2, outs
    import re
    parsed = [[ast.literal_eval(m) for m in re.findall(r"\[[^\]]*\]", r)] for r in rows]
    for (err, slot, pad), _head, _total in parsed:
        # a / 2 + b / 2 in fp32: the halves are exact, the sum is rounded once: half an ulp (2^-22) of a value below 4
        assert err <= 2.0 ** -23 and slot == 3.0 and pad == 0.0, (err, slot, pad)
    assert parsed[0][1] == parsed[1][1] and parsed[0][2] == parsed[1][2]         # identical on both ranks
