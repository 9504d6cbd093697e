// SE(3) in fp64: the one home of rigid-transform arithmetic for every kernel that handles a pose (odometry_eval.hip,
// stream_state.hip, keyframe.hip, icp.hip, projective.hip, voxel_map.hip, pose_graph.hip).  A pose is rows 0..2 of a
// homogeneous transform; here are its products, its two inverses, its action on a point and on a direction, the two ways
// to write it back into a 4x4 matrix, the unit quaternion of its rotation and the reference's pose rows.  One body per
// operation, a fixed order of evaluation in each (the library is built with -ffp-contract=off), so every caller gets the
// same bits.  The pure functions are host+device: a stand-alone host program can print what the kernels compute.
#pragma once
#include <math.h>

#include "common.hpp"

namespace pwclo {

#define SE3_HD __host__ __device__ __forceinline__

struct Se3 {           // rows 0..2 of a homogeneous transform, row-major: r[4*i + j], j = 3 is the translation
  double m[12];
};
struct Quat { double w, x, y, z; };

SE3_HD Se3 se3_identity() {
  Se3 a;
#pragma unroll
  for (int i = 0; i < 12; ++i) a.m[i] = (i % 5 == 0) ? 1.0 : 0.0;
  return a;
}
// c = a . b
SE3_HD Se3 se3_mul(const Se3 &a, const Se3 &b) {
  Se3 c;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double s = a.m[4 * i + 0] * b.m[j] + a.m[4 * i + 1] * b.m[4 + j] + a.m[4 * i + 2] * b.m[8 + j];
      if (j == 3) s += a.m[4 * i + 3];
      c.m[4 * i + j] = s;
    }
  }
  return c;
}
// Two inverses.  se3_rigid_inv is [R^T | -R^T t]: exact for a rotation, and what the registration and pose-graph kernels
// use on poses they keep orthonormal themselves.  se3_inv is the general inverse of [A t; 0 1] (A^-1 by cofactors,
// -A^-1 t): for matrices that come from outside (ground-truth files may hold anything; quat2mat of a non-unit quaternion is
// still a rotation), where A need not be orthonormal.
SE3_HD Se3 se3_rigid_inv(const Se3 &a) {
  Se3 r;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) r.m[4 * i + j] = a.m[4 * j + i];
    r.m[4 * i + 3] = -((a.m[i] * a.m[3] + a.m[4 + i] * a.m[7]) + a.m[8 + i] * a.m[11]);
  }
  return r;
}
SE3_HD Se3 se3_inv(const Se3 &a) {
  const double a00 = a.m[0], a01 = a.m[1], a02 = a.m[2], a10 = a.m[4], a11 = a.m[5], a12 = a.m[6], a20 = a.m[8],
               a21 = a.m[9], a22 = a.m[10];
  const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
  const double det = a00 * c00 + a01 * c01 + a02 * c02;
  const double id = 1.0 / det;
  Se3 r;
  r.m[0] = c00 * id; r.m[1] = (a02 * a21 - a01 * a22) * id; r.m[2] = (a01 * a12 - a02 * a11) * id;
  r.m[4] = c01 * id; r.m[5] = (a00 * a22 - a02 * a20) * id; r.m[6] = (a02 * a10 - a00 * a12) * id;
  r.m[8] = c02 * id; r.m[9] = (a01 * a20 - a00 * a21) * id; r.m[10] = (a00 * a11 - a01 * a10) * id;
#pragma unroll
  for (int i = 0; i < 3; ++i)
    r.m[4 * i + 3] = -(r.m[4 * i] * a.m[3] + r.m[4 * i + 1] * a.m[7] + r.m[4 * i + 2] * a.m[11]);
  return r;
}
// o = a p (the point) and o = R_a v (a direction: rows .[0..2] only), in fp64
SE3_HD void se3_apply(const Se3 &a, const float p[3], double o[3]) {
  const double x = p[0], y = p[1], z = p[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = ((a.m[4 * i] * x + a.m[4 * i + 1] * y) + a.m[4 * i + 2] * z) + a.m[4 * i + 3];
}
SE3_HD void se3_rotate(const Se3 &a, const double v[3], double o[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = (a.m[4 * i] * v[0] + a.m[4 * i + 1] * v[1]) + a.m[4 * i + 2] * v[2];
}
SE3_HD Se3 se3_load(const double *p) {   // from a 4x4 row-major matrix
  Se3 a;
#pragma unroll
  for (int i = 0; i < 12; ++i) a.m[i] = p[i];
  return a;
}
// Into a 4x4 row-major matrix: se3_store writes all 16 words (rows 0..2, then 0 0 0 1), se3_store_rows rows 0..2 only and
// leaves the caller's row 3 alone.  Which words a kernel writes is part of what it does: keep the form a call site has.
SE3_HD void se3_store_rows(double *p, const Se3 &a) {
#pragma unroll
  for (int i = 0; i < 12; ++i) p[i] = a.m[i];
}
SE3_HD void se3_store(double *p, const Se3 &a) {
  se3_store_rows(p, a);
  p[12] = 0.0; p[13] = 0.0; p[14] = 0.0; p[15] = 1.0;
}
__device__ __forceinline__ Se3 se3_shfl_up(const Se3 &a, int delta) {
  Se3 r;
#pragma unroll
  for (int i = 0; i < 12; ++i) r.m[i] = __shfl_up(a.m[i], delta, 64);
  return r;
}
__device__ __forceinline__ double f64_shfl_up(double v, int delta) { return __shfl_up(v, delta, 64); }

// train.py:762-795 (quat2mat: the nibabel form, valid for non-unit quaternions, identity below 1e-8) and
// :873-878: T = [[R t], [0 0 0 1]] from a pose row [tx ty tz qw qx qy qz].  fp32 inputs, fp64 arithmetic.
SE3_HD Se3 pose_row_to_se3(const float *r) {
  const double w = r[3], x = r[4], y = r[5], z = r[6];
  const double nq = w * w + x * x + y * y + z * z;
  Se3 a = se3_identity();
  if (!(nq < 1e-8)) {
    const double s = 2.0 / nq;
    const double X = x * s, Y = y * s, Z = z * s;
    const double wX = w * X, wY = w * Y, wZ = w * Z, xX = x * X, xY = x * Y, xZ = x * Z, yY = y * Y, yZ = y * Z,
                 zZ = z * Z;
    a.m[0] = 1.0 - (yY + zZ); a.m[1] = xY - wZ; a.m[2] = xZ + wY;
    a.m[4] = xY + wZ; a.m[5] = 1.0 - (xX + zZ); a.m[6] = yZ - wX;
    a.m[8] = xZ - wY; a.m[9] = yZ + wX; a.m[10] = 1.0 - (xX + yY);
  }
  a.m[3] = r[0]; a.m[7] = r[1]; a.m[11] = r[2];
  return a;
}

// The unit quaternion of a's rotation by Shepperd's branch selection: the largest of the trace and the three diagonal
// entries decides which component is taken from a square root, so no branch divides by a small number; then normalised.
// No sign rule (w may be negative) and no rounding.
SE3_HD Quat se3_quat(const Se3 &a) {
  const double r00 = a.m[0], r01 = a.m[1], r02 = a.m[2], r10 = a.m[4], r11 = a.m[5], r12 = a.m[6], r20 = a.m[8],
               r21 = a.m[9], r22 = a.m[10];
  const double tr = (r00 + r11) + r22;
  double w, x, y, z;
  if (tr >= r00 && tr >= r11 && tr >= r22) {
    const double u = sqrt(1.0 + tr), k = 0.5 / u;
    w = 0.5 * u; x = (r21 - r12) * k; y = (r02 - r20) * k; z = (r10 - r01) * k;
  } else if (r00 >= r11 && r00 >= r22) {
    const double u = sqrt(((1.0 + r00) - r11) - r22), k = 0.5 / u;
    x = 0.5 * u; w = (r21 - r12) * k; y = (r01 + r10) * k; z = (r02 + r20) * k;
  } else if (r11 >= r22) {
    const double u = sqrt(((1.0 - r00) + r11) - r22), k = 0.5 / u;
    y = 0.5 * u; w = (r02 - r20) * k; x = (r01 + r10) * k; z = (r12 + r21) * k;
  } else {
    const double u = sqrt(((1.0 - r00) - r11) + r22), k = 0.5 / u;
    z = 0.5 * u; w = (r10 - r01) * k; x = (r02 + r20) * k; y = (r12 + r21) * k;
  }
  const double inv = 1.0 / sqrt(((w * w + x * x) + y * y) + z * z);
  return Quat{w * inv, x * inv, y * inv, z * inv};
}

// The other way: the pose row [tx ty tz qw qx qy qz] of a rigid transform: se3_quat, turned so that w >= 0, every
// component rounded to fp32 once.  The sign is applied after the normalisation, -(c * inv) where c * (-inv) would also
// do: a negation is exact, so both give the same bits.  (w < 0 is read off the normalised w, which has the sign of the
// branch's w unless w * inv underflows to -0: that needs 0 < -w < 2.5e-324 |q| with |q| > 2 before normalisation, which
// no pose has.)
SE3_HD void se3_to_pose_row(const Se3 &a, float *r) {
  const Quat q = se3_quat(a);
  const bool neg = q.w < 0.0;
  r[0] = (float)a.m[3]; r[1] = (float)a.m[7]; r[2] = (float)a.m[11];
  r[3] = (float)(neg ? -q.w : q.w); r[4] = (float)(neg ? -q.x : q.x); r[5] = (float)(neg ? -q.y : q.y);
  r[6] = (float)(neg ? -q.z : q.z);
}

}  // namespace pwclo
