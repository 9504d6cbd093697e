// Layout constants and SE(3) helpers of the pose-graph backend (pose_graph.hip).  All fp64; every
// expression is written in the order tests/pose_graph_model.py evaluates it (the library is built with -ffp-contract=off).
#pragma once
#include "common.hpp"
#include "se3.hpp"

namespace pwclo {

constexpr int PG_MAX_STREAMS = 1024;
constexpr int PG_THREADS = 256;        // the workgroup of solve and judge: one per stream (four waves: fp64 6 x 6 blocks stay in registers)
constexpr int PG_RED = PG_THREADS / 64 + 1;   // doubles of LDS a fixed-order sum uses: one per wave and the result
constexpr int PG_EDGE_THREADS = 64;    // linearise: one thread per edge
// one edge's slot of doubles: e, Omega e, Ji^T Omega Ji, Ji^T Omega Jj, Jj^T Omega Jj, Ji^T Omega e, Jj^T Omega e, chi2
constexpr int PG_E = 0, PG_OE = 6, PG_HII = 12, PG_HIJ = 48, PG_HJJ = 84, PG_BI = 120, PG_BJ = 126, PG_CHI = 132;
constexpr int PG_SLOT = 136;
// sections of the solver's workspace, each (S, N, 6) doubles but the last, (S, N, 36)
constexpr int PG_W_R = 0, PG_W_Z = 1, PG_W_P = 2, PG_W_AP = 3, PG_W_G = 4, PG_W_MINV = 5;
constexpr int PG_WORK_PER_VERTEX = 5 * 6 + 36;
// status bits (an active stream with a non-zero word is frozen for the rest of the call)
constexpr int PG_CONVERGED = 1, PG_TRIVIAL = 2, PG_NONFINITE = 4;   // (an idle stream keeps its word: there is no idle bit)

struct PgQuat { double w, x, y, z; };

// Unit quaternion of a rotation by Shepperd's branch selection (se3_to_pose_row's, without its rounding and without the
// sign rule: w may be negative).
__device__ __forceinline__ PgQuat pg_quat(const Se3 &a) {
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
  return PgQuat{w * inv, x * inv, y * inv, z * inv};
}

// The rotation of a unit quaternion into rows 0..2 of a (its translation stays).
__device__ __forceinline__ void pg_set_rotation(Se3 &a, const PgQuat &q) {
  const double xx = q.x * q.x, yy = q.y * q.y, zz = q.z * q.z, xy = q.x * q.y, xz = q.x * q.z, yz = q.y * q.z,
               wx = q.w * q.x, wy = q.w * q.y, wz = q.w * q.z;
  a.m[0] = 1.0 - 2.0 * (yy + zz); a.m[1] = 2.0 * (xy - wz); a.m[2] = 2.0 * (xz + wy);
  a.m[4] = 2.0 * (xy + wz); a.m[5] = 1.0 - 2.0 * (xx + zz); a.m[6] = 2.0 * (yz - wx);
  a.m[8] = 2.0 * (xz - wy); a.m[9] = 2.0 * (yz + wx); a.m[10] = 1.0 - 2.0 * (xx + yy);
}

// Inverse of a rigid transform: R^T, -R^T t.
__device__ __forceinline__ Se3 pg_rigid_inv(const Se3 &a) {
  Se3 r;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) r.m[4 * i + j] = a.m[4 * j + i];
    r.m[4 * i + 3] = -((a.m[i] * a.m[3] + a.m[4 + i] * a.m[7]) + a.m[8 + i] * a.m[11]);
  }
  return r;
}

// X . D(delta), delta = (rho, nu): D = [R(q), rho], q = (sqrt(1 - |nu|^2), nu), or (0, nu / |nu|) where |nu|^2 > 1; the
// product's rotation is then rebuilt from its normalised quaternion.
__device__ __forceinline__ Se3 pg_retract(const Se3 &x, const double *d) {
  const double n2 = (d[3] * d[3] + d[4] * d[4]) + d[5] * d[5];
  PgQuat q;
  if (n2 > 1.0) {
    const double inv = 1.0 / sqrt(n2);
    q = PgQuat{0.0, d[3] * inv, d[4] * inv, d[5] * inv};
  } else {
    q = PgQuat{sqrt(1.0 - n2), d[3], d[4], d[5]};
  }
  Se3 D;
  pg_set_rotation(D, q);
  D.m[3] = d[0]; D.m[7] = d[1]; D.m[11] = d[2];
  Se3 t = se3_mul(x, D);
  pg_set_rotation(t, pg_quat(t));
  return t;
}

}  // namespace pwclo
