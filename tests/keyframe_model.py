"""NumPy fp64 model of the keyframe gate and of the gated map bookkeeping, and of the pose row the
refined motion is handed to the de-skew prior in.  The gate restates the reference's ``__update_map``
(slam/odometry/icp_odometry.py:361-381) by reading it -- the motion since the last inserted frame is accumulated, the frame
is inserted when that motion exceeds a translation or a rotation threshold (both strict), otherwise the map is only moved
into the new frame -- with one deliberate departure: the rotation is measured by its angle, not by the norm of its Euler
angles.  The reference itself is not run."""
import numpy as np

import icp_model as model


def measure(D):
    """-> (|D[:3, 3]| in metres, the rotation angle of D in degrees as atan2(s, c))."""
    R = D[:3, :3]
    c = 0.5 * (((R[0, 0] + R[1, 1]) + R[2, 2]) - 1.0)
    ax, ay, az = R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]
    s = 0.5 * np.sqrt((ax * ax + ay * ay) + az * az)
    t = np.sqrt((D[0, 3] * D[0, 3] + D[1, 3] * D[1, 3]) + D[2, 3] * D[2, 3])
    return float(t), float(np.arctan2(s, c) * (180.0 / np.pi))


class Gate:
    """One stream's gate: delta (4, 4), insert, count."""

    def __init__(self, trans, rot):
        self.trans, self.rot = float(trans), float(rot)
        self.delta, self.insert, self.count = np.eye(4), 0, 0

    def step(self, T, any_live, active=True):
        """The decision for a frame registered with T against a map with (``any_live``) or without a live slot -> insert."""
        if not active:
            self.insert = 0
            return 0
        if not any_live:
            self.delta, self.insert, self.count = np.eye(4), 1, 1
            return 1
        D = self.delta @ np.asarray(T, dtype=np.float64)
        t, angle = measure(D)
        if t > self.trans or angle > self.rot:
            self.delta, self.insert = np.eye(4), 1
            self.count += 1
        else:
            self.delta, self.insert = D, 0
        return self.insert

    def margin(self, T, any_live):
        """How far, relatively, the frame's measures stay from the thresholds (inf where a threshold is 0 or no comparison
        is made): a test draws its inputs so that this exceeds the rounding of the device's fp64 arithmetic."""
        if not any_live:
            return np.inf
        t, angle = measure(self.delta @ np.asarray(T, dtype=np.float64))
        rel = lambda v, th: abs(v - th) / th if th > 0 else np.inf
        return min(rel(t, self.trans), rel(angle, self.rot))


def push(mp, cloud, T, insert, normals32=None):
    """``icp_model.Map.push`` behind the gate: insert -> that push; otherwise every live slot, the cursor's included, is
    re-based (A <- A T, R <- R_T^T R) and nothing else changes."""
    if insert:
        mp.push(cloud, T, normals32)
        return
    for m in range(mp.M):
        if mp.live[m]:
            mp.A[m] = mp.A[m] @ T
            mp.R[m] = T[:3, :3].T @ mp.R[m]


def pose_row(T):
    """The pose row [tx ty tz qw qx qy qz] of a rigid transform in fp64, before the one rounding to fp32: Shepperd's branch
    selection, normalised, w >= 0."""
    R = np.asarray(T, dtype=np.float64)[:3, :3]
    r00, r01, r02, r10, r11, r12, r20, r21, r22 = R.reshape(9)
    tr = (r00 + r11) + r22
    if tr >= r00 and tr >= r11 and tr >= r22:
        u = np.sqrt(1.0 + tr)
        k = 0.5 / u
        q = [0.5 * u, (r21 - r12) * k, (r02 - r20) * k, (r10 - r01) * k]
    elif r00 >= r11 and r00 >= r22:
        u = np.sqrt(((1.0 + r00) - r11) - r22)
        k = 0.5 / u
        q = [(r21 - r12) * k, 0.5 * u, (r01 + r10) * k, (r02 + r20) * k]
    elif r11 >= r22:
        u = np.sqrt(((1.0 - r00) + r11) - r22)
        k = 0.5 / u
        q = [(r02 - r20) * k, (r01 + r10) * k, 0.5 * u, (r12 + r21) * k]
    else:
        u = np.sqrt(((1.0 - r00) - r11) + r22)
        k = 0.5 / u
        q = [(r10 - r01) * k, (r02 + r20) * k, (r12 + r21) * k, 0.5 * u]
    q = np.array(q)
    inv = 1.0 / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    if q[0] < 0.0:
        inv = -inv
    return np.concatenate([np.asarray(T, dtype=np.float64)[:3, 3], q * inv])


def small(r, trans, deg):
    """A random motion of ``trans`` metres and ``deg`` degrees."""
    d = r.normal(size=3)
    return model.pose(model.rot(r.normal(size=3), np.deg2rad(deg)), trans * d / np.linalg.norm(d))


# ---- scenes: icp_model's box room walked with motions the caller chooses ----------------------------------------------------

def steps(translations, deg=0.1):
    """Per-frame motions: ``translations`` metres along a fixed direction, ``deg`` degrees about a fixed tilted axis."""
    d = np.array([0.96, 0.28, 0.0])
    return [model.pose(model.rot([0.3, -0.2, 1.0], np.deg2rad(deg)), t * d) for t in translations]


def room_walk(seed, motions, n, noise=0.01):
    """``icp_model.room`` with the caller's motions: frame 0 at the origin, frame k + 1 = frame k moved by ``motions[k]``;
    every frame samples its own n ray directions and gets its own range noise.
    -> (clouds (frames, n, 3) fp32 in the sensor frames, T (frames, 4, 4): T[k] maps frame k into frame k - 1, T[0] = I)."""
    r = np.random.default_rng([seed, len(motions), n])
    world = [np.eye(4)]
    for step in motions:
        world.append(world[-1] @ step)
    clouds = np.empty((len(world), n, 3), dtype=np.float32)
    for k, W in enumerate(world):
        pts = np.empty((0, 3))
        while pts.shape[0] < n:
            d = r.normal(size=(2 * n, 3))
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            dw = d @ W[:3, :3].T
            with np.errstate(divide="ignore"):
                t = np.where(dw > 0, (model.ROOM - W[:3, 3]) / dw, (-model.ROOM - W[:3, 3]) / dw)
            rng = t.min(axis=1)
            keep = np.isfinite(rng)
            pts = np.concatenate([pts, (d * (rng + r.normal(0.0, noise, len(d)))[:, None])[keep]])
        clouds[k] = pts[:n]
    return clouds, np.stack([np.eye(4)] + [np.asarray(m, dtype=np.float64) for m in motions])


# Six frames per stream for the whole-refiner tests, thresholds trans = 0.15 m, rot = 5 degrees: frame 0 fills the map,
# frame 1 crosses alone, frames 2-3 stay below, frame 4 crosses by accumulation only, frame 5 crosses alone.
WALK_KEYFRAME = dict(trans=0.15, rot=5.0)
WALK = [[0.30, 0.04, 0.04, 0.12, 0.30], [0.25, 0.05, 0.03, 0.11, 0.28]]
WALK_INSERTS = [1, 1, 0, 0, 1, 1]
