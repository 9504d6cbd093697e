// Layout constants of the pose-graph backend (pose_graph.hip) and its retraction.  Products, the
// rigid inverse and the quaternion of a rotation are se3.hpp's; here are only the rotation of a quaternion and the step
// X . D(delta) built on them.  All fp64; every expression is written in the order tests/pose_graph_model.py evaluates it
// (the library is built with -ffp-contract=off).
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
// the slot's spare doubles, written by the robust linearise alone: the raw e^T Omega e and the weight rho'(c) (PG_CHI is rho)
constexpr int PG_RAW = 133, PG_W = 134;
// robust kernels (section 25.1): one kind and one delta per graph, applied to the edge classes of a mask
constexpr int PG_ROBUST_NONE = 0, PG_HUBER = 1, PG_GEMAN_MCCLURE = 2, PG_DCS = 3;
constexpr int PG_CLASS_CHAIN = 1, PG_CLASS_LOOP = 2, PG_CLASS_ABSOLUTE = 4;
// sections of the solver's workspace, each (S, N, 6) doubles but the last, (S, N, 36)
constexpr int PG_W_R = 0, PG_W_Z = 1, PG_W_P = 2, PG_W_AP = 3, PG_W_G = 4, PG_W_MINV = 5;
constexpr int PG_WORK_PER_VERTEX = 5 * 6 + 36;
// status bits (an active stream with a non-zero word is frozen for the rest of the call)
constexpr int PG_CONVERGED = 1, PG_TRIVIAL = 2, PG_NONFINITE = 4;   // (an idle stream keeps its word: there is no idle bit)

// rho(c) and w = rho'(c) of a robust kernel at the raw term c = e^T Omega e, each expression in the order of
// tests/pose_graph_robust_model.py.  A non-finite c gives a non-finite rho with every kind, so the solve still reports it.
__host__ __device__ __forceinline__ void pg_robustify(int kind, double delta, double c, double *rho, double *w) {
  if (kind == PG_HUBER) {
    if (c <= delta * delta) {
      *rho = c; *w = 1.0;
    } else {
      const double s = sqrt(c);
      *rho = (2.0 * s) * delta - delta * delta;
      *w = delta / s;
    }
  } else if (kind == PG_GEMAN_MCCLURE) {
    const double a = delta / (delta + c);
    *rho = c * a;
    *w = a * a;
  } else if (kind == PG_DCS) {
    const double s = (2.0 * delta) / (delta + c);
    if (s >= 1.0) {
      *rho = c; *w = 1.0;
    } else {
      *w = s * s;
      *rho = *w * c;
    }
  } else {
    *rho = c; *w = 1.0;
  }
}

// The rotation of a unit quaternion into rows 0..2 of a (its translation stays).
__device__ __forceinline__ void pg_set_rotation(Se3 &a, const Quat &q) {
  const double xx = q.x * q.x, yy = q.y * q.y, zz = q.z * q.z, xy = q.x * q.y, xz = q.x * q.z, yz = q.y * q.z,
               wx = q.w * q.x, wy = q.w * q.y, wz = q.w * q.z;
  a.m[0] = 1.0 - 2.0 * (yy + zz); a.m[1] = 2.0 * (xy - wz); a.m[2] = 2.0 * (xz + wy);
  a.m[4] = 2.0 * (xy + wz); a.m[5] = 1.0 - 2.0 * (xx + zz); a.m[6] = 2.0 * (yz - wx);
  a.m[8] = 2.0 * (xz - wy); a.m[9] = 2.0 * (yz + wx); a.m[10] = 1.0 - 2.0 * (xx + yy);
}

// X . D(delta), delta = (rho, nu): D = [R(q), rho], q = (sqrt(1 - |nu|^2), nu), or (0, nu / |nu|) where |nu|^2 > 1; the
// product's rotation is then rebuilt from its normalised quaternion.
__device__ __forceinline__ Se3 pg_retract(const Se3 &x, const double *d) {
  const double n2 = (d[3] * d[3] + d[4] * d[4]) + d[5] * d[5];
  Quat q;
  if (n2 > 1.0) {
    const double inv = 1.0 / sqrt(n2);
    q = Quat{0.0, d[3] * inv, d[4] * inv, d[5] * inv};
  } else {
    q = Quat{sqrt(1.0 - n2), d[3], d[4], d[5]};
  }
  Se3 D;
  pg_set_rotation(D, q);
  D.m[3] = d[0]; D.m[7] = d[1]; D.m[11] = d[2];
  Se3 t = se3_mul(x, D);
  pg_set_rotation(t, se3_quat(t));
  return t;
}

}  // namespace pwclo
