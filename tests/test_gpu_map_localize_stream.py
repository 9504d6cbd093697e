"""GPU tests of ``StreamingOdometry(map=..., localize=...)`` at S = 2 on frames of
``loop_closure_cases.revisit()``: localisation changes no existing output, freezes with the few-pairs bit while no old part
of the map may attract, equals a stand-alone ``MapLocalizer`` fed the same words, hands exactly the converged fixes to the
pose graph as absolute edges, and leaves an idle stream's words alone.

The suite's network says "no motion", so the source trajectory is the identity throughout: a revisit under that trajectory
is a frame that sees what an old frame saw.  Stream 0 is fed frame 0 again in call 8 (the same place); stream 1 is fed the
scene's other place.  ``min_id_distance`` = 8, so in every call before the revisit the gate hides the whole map, and in the
revisit only frame 0 attracts."""
import functools

import numpy as np
import pytest
import torch

import loop_closure_cases as LC
from oracle import params
from pwclonet_pylidarslam_amd.map_localize import MapLocalizer
from pwclonet_pylidarslam_amd.odometry import StreamingOdometry
from pwclonet_pylidarslam_amd.pwclonet import PWCLONet

pytestmark = pytest.mark.gpu
S, N, V, MIN_ID = 2, LC.REVISIT_N, 0.3, 8
FEW_PAIRS, CONVERGED, IDLE = 2, 1, 8


@functools.lru_cache(maxsize=None)
def _net(dev):
    """The suite's synthetic weights with every pose head's last layer set to "no motion" (tests/test_gpu_icp_masked.py)."""
    net = PWCLONet(dict(num_input_channels=3, sequence_len=2, device=str(dev), scalar_last=False, log_mode="none",
                        fused="auto"))
    sd = net.state_dict()
    params.fill_state_dict(sd)
    for key, v in sd.items():
        if key.endswith(("conv1d_q.conv.weight", "conv1d_t.conv.weight", "conv1d_t.conv.bias")):
            v.zero_()
        elif key.endswith("conv1d_q.conv.bias"):
            v.copy_(torch.tensor([1.0, 0.0, 0.0, 0.0]))
    net = net.to(dev).eval()
    net.prepare_fused()
    return net


@functools.lru_cache(maxsize=None)
def _calls():
    """Nine calls of (S, N, 4) frames: the scene's frames 0..7, then the revisit."""
    f = LC.revisit()["frames"]
    order = [(k, k) for k in range(8)] + [(0, 39)]
    out = []
    for a, b in order:
        x = np.zeros((S, N, 4), dtype=np.float32)
        x[0, :, :3], x[1, :, :3] = f[a, 0], f[b, 1]
        out.append(x)
    return out


def test_lock_step_localisation_in_the_map(cuda):
    net, calls = _net(cuda), _calls()
    kw = dict(streams=S, max_frames=16, backend=dict(source="network", max_loops=4, iters=6),
              map=dict(voxel_size=V, max_keyframes=16))
    plain = StreamingOdometry(net, **kw)
    local = StreamingOdometry(net, localize=dict(min_id_distance=MIN_ID, radius=2, min_pairs=64), **kw)
    alone = None
    handed = []
    eye = torch.eye(4, dtype=torch.float64, device=cuda).expand(S, 4, 4).contiguous()
    with torch.no_grad():
        for c, frames in enumerate(calls):
            frames = torch.from_numpy(frames).to(cuda)
            a, b = plain.step(frames), local.step(frames)
            assert (a is None and b is None) or torch.equal(a, b)
            if c == 0:
                assert local.localizer() is None and local.localized_pose() is None and local.localized_status() is None
                assert local.poll_localization() == []
                continue
            # a localiser of its own, fed the same words: the frame's pose in the source trajectory, the same gate.  The map
            # has banked frame c by now; the gate hides it, and older points never move when a frame is appended.
            alone = alone or MapLocalizer(local.global_map(), radius=2, min_pairs=64, graph=False)
            alone.index()
            init = local.optimized_trajectory()[c].clone()
            want = alone.localize(frames[:, :N, :3].contiguous(), init, max_source_frame=[c - MIN_ID] * S)
            status = local.localized_status().tolist()
            pairs = local.localizer().diagnostics()["pairs"].tolist()
            print("call %d: status %s pairs %s" % (c, status, pairs))
            assert torch.equal(local.localized_pose(), want), c
            assert status == alone.status().tolist() and pairs == alone.diagnostics()["pairs"].tolist()
            if c < len(calls) - 1:                       # every call before the revisit: nothing old enough to attract
                assert c < MIN_ID and status == [FEW_PAIRS] * S and pairs == [0] * S
            before = [len(e) for e in local.backend()._abs]
            ran = local.backend().calls
            fixes = local.poll_localization(optimize=True)
            expect = [s for s in range(S) if status[s] == CONVERGED and pairs[s] >= 64]
            assert [f[0] for f in fixes] == expect and all(f[1] == c for f in fixes), (c, status, pairs)
            assert all(np.array_equal(f[2], want[f[0]].cpu().numpy()) for f in fixes)
            assert [len(e) for e in local.backend()._abs] == [before[s] + (s in expect) for s in range(S)]
            assert local.backend().calls == ran + (1 if expect else 0)           # optimize ran where a fix was handed over
            assert local.poll_localization(optimize=True) == []                 # once per step
            handed += [(c,) + f for f in fixes]
    assert (len(calls) - 1, 0) in [(f[0], f[1]) for f in handed]                 # the revisit of stream 0 is a fix
    assert not any(f[1] == 1 and f[0] == len(calls) - 1 for f in handed)         # the other place is none
    for name in ("relative_poses", "trajectory"):
        assert torch.equal(getattr(plain, name)(), getattr(local, name)()), name
    assert local.captures == plain.captures and local.localizer().captures == 1
    with pytest.raises(ValueError, match="needs map="):
        StreamingOdometry(net, streams=S, localize=dict())
    with pytest.raises(RuntimeError, match="needs backend="):
        StreamingOdometry(net, streams=S, map=dict(), localize=dict()).poll_localization()


def test_per_stream_localisation_with_a_dropout_and_a_restart(cuda):
    net, calls = _net(cuda), _calls()
    active = np.array([[1, 1], [1, 1], [1, 0], [1, 1], [1, 1], [1, 1], [1, 1]], dtype=np.int32)
    restart = np.zeros_like(active)
    restart[4, 0] = 1
    kw = dict(streams=S, max_frames=16, per_stream=True, map=dict(voxel_size=V, max_keyframes=16))
    plain = StreamingOdometry(net, **kw)
    local = StreamingOdometry(net, localize=dict(min_id_distance=2, radius=2), **kw)
    with torch.no_grad():
        for c in range(len(active)):
            frames = torch.from_numpy(calls[c]).to(cuda)
            act, rst = active[c].tolist(), torch.from_numpy(restart[c]).to(cuda)
            keep = None if local.localizer() is None else (local.localized_pose().clone(),)
            a, b = plain.step(frames, active=act, restart=rst), local.step(frames, active=act, restart=rst)
            assert torch.equal(a, b) and torch.equal(plain.frame_counts(), local.frame_counts())
            for s in range(S):
                for name in ("relative_poses", "trajectory"):
                    assert torch.equal(getattr(plain, name)(stream=s), getattr(local, name)(stream=s)), (c, s, name)
                assert torch.equal(plain.global_map().points(s), local.global_map().points(s)), (c, s)
            if c == 2:                                   # stream 1 delivered nothing: its pose word for word, status idle
                assert local.localized_status().tolist()[1] == IDLE and torch.equal(local.localized_pose()[1], keep[0][1])
            if c == 4:                                   # stream 0 starts a new sequence: frame id 0, nothing old to attract
                assert local.localized_status().tolist()[0] == FEW_PAIRS
    loc, fresh = local.localizer(), MapLocalizer(local.global_map(), radius=2, graph=False)
    # call 5 indexed stream 0 from rank 0 (its map was emptied by call 4), call 6 appended; the map has banked one frame since
    fresh.index()
    live = (fresh.bufs["index"][0] >= 0) & (fresh.bufs["index"][0] < loc.indexed()[0])      # what call 6's pass had seen
    assert int(live.sum()) == int(loc.indexed()[0]) > 0
    assert torch.equal(loc.bufs["index"][0][live], fresh.bufs["index"][0][live])  # every rank of the new map is findable
    assert local.captures == plain.captures == 1
