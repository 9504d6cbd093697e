"""Shared by tests/test_gpu_pipeline_priority.py and, run as a program, its child process.

``PWCLO_PIPE_PRIORITY`` is read once per process, so every value needs a process of its own:

    python tests/pipe_priority_cases.py

takes the value from its environment, runs ``PipelinedForward`` at depth 4 for 9 calls on 9 different inputs (batch 2,
2 x 1024 points: the smallest shape of the suite's forwards, and 9 = 2 * 4 + 1 wraps the slot rotation twice with a
remainder for any lane count from 1 to 4), compares every pose byte for byte with a serial ``GraphedForward`` on the same
input, prints one ``RESULT {json}`` line and exits 1 on any difference."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

VALUES = ("normal", "high", "low", "mixed", "auto")
DEPTH, CALLS, BATCH, NPOINTS = 4, 9, 2, 1024


def make_net(dev):
    from oracle import params
    from pwclonet_pylidarslam_amd.pwclonet import PWCLONet
    net = PWCLONet(dict(num_input_channels=3, sequence_len=2, device=str(dev), scalar_last=False, log_mode="none"))
    params.fill_state_dict(net.state_dict())
    net = net.to(dev).eval()
    net.prepare_fused()
    return net


def make_inputs(dev):
    """CALLS input pairs, all different."""
    import torch
    from pwclonet_pylidarslam_amd import synthetic
    out = []
    for c in range(CALLS):
        pc1, pc2, _, _ = synthetic.kitti_like_pair(300 + c, NPOINTS, BATCH)
        out.append(tuple(torch.from_numpy(p[:, :, :3]).permute(0, 2, 1).contiguous().to(dev) for p in (pc1, pc2)))
    return out


def serial_poses(net, inputs):
    import torch
    from pwclonet_pylidarslam_amd.graphed import GraphedForward
    g = GraphedForward(net)
    refs = [g(a, b).clone() for a, b in inputs]
    torch.cuda.synchronize()
    for i in range(1, len(refs)):
        assert not torch.equal(refs[0], refs[i]), "inputs 0 and %d give one pose: the check could not tell calls apart" % i
    return refs


def pipelined_poses(net, inputs):
    """-> (pipe, [pose of call c]): nothing is waited for between the calls; every output is cloned on its slot's stream
    behind the replay (the slot's buffer is overwritten DEPTH calls later)."""
    import torch
    from pwclonet_pylidarslam_amd.graphed import PipelinedForward
    pipe = PipelinedForward(net, depth=DEPTH)
    got = []
    for c, (a, b) in enumerate(inputs):
        out, slot = pipe(a, b)
        assert slot == c % DEPTH
        with torch.cuda.stream(pipe._where[slot]):
            got.append(out.clone())
    pipe.wait_all()
    return pipe, got


def consistent(d):
    """What ``describe()`` must satisfy on the native set at depth 4: the lanes are the probe's value of the very layout
    it names, their indices are among the streams that ran together, and a layout other than normal is only ever chosen
    by ``auto`` when all four streams ran side by side in it."""
    ok = d["streams"] == "native" and d["layout"] in VALUES[:4] and d["follows_probe"] is True
    ok = ok and d["lanes"] == min(DEPTH, d["side_by_side"]) == len(d["stream_indices"])
    ok = ok and list(d["stream_indices"]) == list(d["together"])[:d["lanes"]] and len(d["together"]) == d["side_by_side"]
    return ok


def main():
    import torch
    from pwclonet_pylidarslam_amd import pipe_streams
    dev = torch.device("cuda:0")
    asked = pipe_streams.priority()
    net = make_net(dev)
    inputs = make_inputs(dev)
    refs = serial_poses(net, inputs)
    pipe, got = pipelined_poses(net, inputs)
    differ = [c for c in range(CALLS) if not torch.equal(got[c], refs[c])]
    d = pipe.describe()
    ok = not differ and consistent(d)
    if asked == "auto":
        ok = ok and (d["layout"] == "normal" or d["side_by_side"] == DEPTH)
    else:       # the layout asked for, or normal where the device has a single priority level
        ok = ok and d["layout"] in (asked, "normal")
    print("RESULT " + json.dumps(dict(asked=asked, differ=differ, ok=ok, **d)))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
