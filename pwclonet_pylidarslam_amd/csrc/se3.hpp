// SE(3) in fp64 for the odometry kernels (odometry_eval.hip, stream_state.hip): rows 0..2 of a homogeneous
// transform, the products the trajectories are built from, and the reference's quat2mat of a pose row.  One body
// for every kernel that turns pose rows into transforms, so their results agree bit for bit.
#pragma once
#include "common.hpp"

namespace pwclo {

struct Se3 {           // rows 0..2 of a homogeneous transform, row-major: r[4*i + j], j = 3 is the translation
  double m[12];
};

__device__ __forceinline__ Se3 se3_identity() {
  Se3 a;
#pragma unroll
  for (int i = 0; i < 12; ++i) a.m[i] = (i % 5 == 0) ? 1.0 : 0.0;
  return a;
}
// c = a . b
__device__ __forceinline__ Se3 se3_mul(const Se3 &a, const Se3 &b) {
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
// General inverse of [A t; 0 1] (A need not be orthonormal: quat2mat of a non-unit quaternion is still a
// rotation, but ground-truth files may hold anything): A^-1 by cofactors, -A^-1 t.
__device__ __forceinline__ Se3 se3_inv(const Se3 &a) {
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
__device__ __forceinline__ Se3 se3_load(const double *p) {   // from a 4x4 row-major matrix
  Se3 a;
#pragma unroll
  for (int i = 0; i < 12; ++i) a.m[i] = p[i];
  return a;
}
__device__ __forceinline__ void se3_store(double *p, const Se3 &a) {
#pragma unroll
  for (int i = 0; i < 12; ++i) p[i] = a.m[i];
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
__device__ __forceinline__ Se3 pose_row_to_se3(const float *r) {
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

// The other way: the pose row [tx ty tz qw qx qy qz] of a rigid transform.  The quaternion comes from the rotation by
// Shepperd's branch selection (the largest of the trace and the three diagonal entries decides which component is taken
// from a square root, so no branch divides by a small number), is normalised, gets w >= 0, and every component is rounded
// to fp32 once.
__device__ __forceinline__ void se3_to_pose_row(const Se3 &a, float *r) {
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
  double inv = 1.0 / sqrt(((w * w + x * x) + y * y) + z * z);
  if (w < 0.0) inv = -inv;
  r[0] = (float)a.m[3]; r[1] = (float)a.m[7]; r[2] = (float)a.m[11];
  r[3] = (float)(w * inv); r[4] = (float)(x * inv); r[5] = (float)(y * inv); r[6] = (float)(z * inv);
}

}  // namespace pwclo
