"""Records tests/golden/projective_cases.npz by running the reference's projective odometry pieces on the CPU.

    python tools/gen_projective_golden.py

Build container only (it needs the reference tree; ``oracle.ref_import`` as it is).  It imports the reference's
``SphericalProjector``, ``compute_normal_map`` and ``compute_neighbors`` (``ProjectiveLocalMap``'s module needs packages
this image lacks well beyond what a stub in this file could stand in for, so ``build_model`` is not recorded) and writes inputs and the
reference's outputs only.  Every cloud holds points at the origin, above and below the field of view, a point with
y = -0.0, x < 0 (column W), several points sharing a pixel with distinct ranges and two identical points; every case has a
``lengths`` shorter than R and an empty cloud.  Conditions enforced by dropping points (asserted afterwards; the share
dropped is printed and must stay below 5 %):
  rounding boundary   every point's fp64 pixel coordinates lie >= 1e-3 px from a rounding boundary / validity limit
  determinant band    no occupied pixel's |det C| (fp64, k = 3 and 5) lies within a factor 4 of 1e-6, and the reference's
                      fp32 decision agrees with the fp64 one there
  neighbour gap       at every associated pixel the best and second-best slot distances differ by >= 1e-4 relative
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_import  # noqa: E402
import icp_model as icp  # noqa: E402
import projective_model as model  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "projective_cases.npz")
CASES = [dict(H=16, W=64, up=3.0, down=-24.8, R=2000, seed=1), dict(H=5, W=60, up=15.0, down=-15.0, R=700, seed=2),
         dict(H=8, W=33, up=3.0, down=-24.8, R=600, seed=3), dict(H=16, W=64, up=15.0, down=-15.0, R=1600, seed=4)]
CLOUDS, BAND, GAP = 3, 1e-3, 1e-4


def load_reference():
    """The reference's modules (``ref_import.load`` installs the stubs these two need)."""
    ref_import.load()
    import importlib
    ns = types.SimpleNamespace()
    ns.projection = importlib.import_module("slam.common.projection")
    ns.geometry = importlib.import_module("slam.common.geometry")
    return ns


def cloud(case, im, r, pose):
    """One cloud (R, 3) fp32 of the box room seen from ``pose``, with the planted rows; -> (points, dropped, offered)."""
    H, W, R = case["H"], case["W"], case["R"]
    n = H * W
    d = model.beams(im, r.uniform(-0.5, 0.5, (n, 2)))
    dw = d @ pose[:3, :3].T
    with np.errstate(divide="ignore"):
        t = np.where(dw > 0, (icp.ROOM - pose[:3, 3]) / dw, (-icp.ROOM - pose[:3, 3]) / dw)
    pts = (d * (t.min(axis=1) + r.normal(0.0, 0.01, n))[:, None])[r.random(n) < 0.9]
    extra = pts[r.integers(0, len(pts), R)] * r.uniform(1.05, 1.6, (R, 1))        # same pixels, distinct ranges
    pts = np.concatenate([pts, extra])[:R - 12].astype(np.float32)
    margin = model.pixels(pts, im)[4]
    ok = margin >= BAND
    dropped, offered = int((~ok).sum()), len(pts)
    pts = pts[ok]
    up, down = np.deg2rad(case["up"]), np.deg2rad(case["down"])
    planted = np.array([[0, 0, 0], [0, 0, 0],
                        [np.cos(up + 0.2), 0.3, np.sin(up + 0.2)], [2 * np.cos(up + 0.5), -1.0, 2 * np.sin(up + 0.5)],
                        [np.cos(down - 0.2), 0.3, np.sin(down - 0.2)], [3 * np.cos(down - 0.4), 1.0, 3 * np.sin(down - 0.4)],
                        [-2.0, -0.0, 0.1], [-3.5, -0.0, -0.2]], dtype=np.float32)
    dup = pts[[5, 5, 40, 40]]                                                   # identical coordinates: the tie rule
    out = np.zeros((R, 3), dtype=np.float32)
    body = np.concatenate([pts[:7], dup[:2], planted, pts[7:], dup[2:]])
    out[:len(body)] = body                                                      # the rest stays at the origin
    return out, dropped, offered


def run_case(ref, case):
    H, W = case["H"], case["W"]
    im = model.image(H, W, case["up"], case["down"])
    proj = ref.projection.SphericalProjector(height=H, width=W, num_channels=3, up_fov=case["up"], down_fov=case["down"])
    r = np.random.default_rng(case["seed"])
    poses = [np.eye(4)] + [icp.pose(icp.rot([0.3, -0.2, 1.0], np.deg2rad(r.uniform(-3, 3))),
                                    np.array([r.uniform(0.1, 0.3), r.uniform(-0.1, 0.1), r.uniform(-0.03, 0.03)]))
                           for _ in range(CLOUDS - 1)]
    world = [poses[0]]
    for p in poses[1:]:
        world.append(world[-1] @ p)
    dropped = offered = 0
    clouds = np.zeros((CLOUDS + 1, case["R"], 3), dtype=np.float32)            # the last cloud stays empty
    for c in range(CLOUDS):
        clouds[c], dr, of = cloud(case, im, r, world[c])
        dropped, offered = dropped + dr, offered + of
    lengths = np.array([case["R"], case["R"] - 37, case["R"] - 5, case["R"]], dtype=np.int32)
    lengths_used = lengths.copy()

    def reference_images(clouds):
        with torch.no_grad():
            vm = [proj.build_projection_map(torch.from_numpy(clouds[c][None, :lengths_used[c]])) for c in range(CLOUDS + 1)]
            nm = {k: [ref.geometry.compute_normal_map(v, kernel_size=k) for v in vm] for k in (3, 5)}
        return vm, nm

    for _ in range(6):                                     # the determinant band: drop the centre point of a pixel in it
        vm, nm = reference_images(clouds)
        bad = 0
        for c in range(CLOUDS):
            v = vm[c][0].permute(1, 2, 0).numpy()
            rows = model.vertex_map(clouds[c], im, lengths_used[c])[1]
            for k in (3, 5):
                n64, det = model.normal_map(v, k)
                occupied = (v != 0).any(axis=-1)
                band = occupied & (np.abs(det) > 1e-6 / 4) & (np.abs(det) < 4e-6)
                differ = occupied & ((nm[k][c][0].permute(1, 2, 0).numpy() != 0).any(axis=-1) != (n64 != 0).any(axis=-1))
                hit = rows[band | differ]
                clouds[c][hit] = 0.0
                bad += hit.size
        dropped += bad
        if bad == 0:
            break
    assert bad == 0, "the determinant band did not clear"

    # neighbours: cloud 0's image as the target, the others as the reference batch
    def neighbours():
        vm, nm = reference_images(clouds)
        with torch.no_grad():
            return vm, nm, ref.geometry.compute_neighbors(vm[0], torch.cat(vm[1:CLOUDS]),
                                                          reference_fields=torch.cat(nm[5][1:CLOUDS]))
    for _ in range(6):
        vm, nm, (nv, nn) = neighbours()
        target = vm[0][0].permute(1, 2, 0).numpy()
        stack = np.stack([v[0].permute(1, 2, 0).numpy() for v in vm[1:CLOUDS]])
        a = model.associate(target, stack, np.ones_like(stack), np.eye(4), im, np.inf)
        close = np.flatnonzero((a["slot"] >= 0) & (a["gap"] < GAP))
        rows = model.vertex_map(clouds[0], im, lengths_used[0])[1].reshape(-1)
        clouds[0][rows[close]] = 0.0
        dropped += close.size
        if close.size == 0:
            break
    assert close.size == 0, "the neighbour gap did not clear"

    out = dict(points=clouds, lengths=lengths, image=np.array([H, W, case["up"], case["down"]], dtype=np.float64))
    with torch.no_grad():
        px = torch.stack([proj.project_pointcloud(torch.from_numpy(clouds[c][None]))[0] for c in range(CLOUDS + 1)])
    out["ref_row"], out["ref_col"] = px[..., 0].round().numpy().astype(np.int32), px[..., 1].round().numpy().astype(np.int32)
    for c in range(CLOUDS + 1):                            # the rounding boundary, asserted on what is written
        mg = model.pixels(clouds[c], im)[4]
        assert (mg[np.isfinite(mg)] >= BAND).all()
    out["ref_vmap"] = np.stack([v[0].permute(1, 2, 0).numpy() for v in vm])
    for k in (3, 5):
        out["ref_nmap%d" % k] = np.stack([v[0].permute(1, 2, 0).numpy() for v in nm[k]])
    out["ref_neighbor_v"] = nv[0].permute(1, 2, 0).numpy()
    out["ref_neighbor_n"] = nn[0].permute(1, 2, 0).numpy()

    return out, dropped, offered


def main():
    # One thread: the reference's scatter into the image lets the last (nearest) write stand only when it runs in order;
    # split across threads, which of several points on one pixel stays is left to chance.
    torch.set_num_threads(1)
    ref = load_reference()
    arrays, dropped, offered = {}, 0, 0
    for i, case in enumerate(CASES):
        out, dr, of = run_case(ref, case)
        dropped, offered = dropped + dr, offered + of
        arrays.update({"c%d_%s" % (i, k): v for k, v in out.items()})
    share = dropped / offered
    print("points dropped by resampling: %d of %d (%.2f %%)" % (dropped, offered, 100.0 * share))
    assert share <= 0.05, "more than 5 %% of the points were dropped"
    arrays["cases"] = np.array(len(CASES))
    np.savez_compressed(OUT, **arrays)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) < (1 << 20)


if __name__ == "__main__":
    main()
