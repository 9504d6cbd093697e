// Row body of the motion compensation of raw sweeps, shared by every kernel that de-skews: the
// stand-alone op and the two fused front ends of deskew.hip.  One definition of the motion, of a row's alpha and of the
// transformed row, so all of them give the same coordinate bits (the pattern rows.hpp exists for).
//
// The rule (the reference's `distortion` filter, slam/preprocessing.py:131-191): row i of a sweep goes to
//   p'_i = R(alpha_i) p_i + alpha_i t,   alpha_i = (tau_i - tau_min) / (tau_max - tau_min)
// with R(alpha) = slerp(I, R, alpha) the rotation by alpha * theta about R's axis and tau_min / tau_max over the kept
// rows with a finite time.  fp64 arithmetic on the fp32 inputs, one rounding to fp32 at the end.
#pragma once
#include <math.h>

#include "common.hpp"

namespace pwclo {

struct DeskewMotion {
  double k[3];          // unit axis
  double theta;         // angle in [0, pi]
  double t[3];
  bool identity;        // theta == 0 and t == 0: every row keeps its bits
};

// A pose row [tx ty tz qw qx qy qz] (fp32) -> the motion; nullptr: the identity.  |q|^2 < 1e-8 is the identity rotation
// (pose_row_to_se3's rule, se3.hpp); otherwise the unit quaternion with w >= 0 (the shortest arc), theta = 2 atan2(|v|, w).
__device__ __forceinline__ DeskewMotion deskew_motion(const float *__restrict__ row) {
  DeskewMotion m;
  m.k[0] = 1.0; m.k[1] = 0.0; m.k[2] = 0.0;
  m.theta = 0.0;
  m.t[0] = 0.0; m.t[1] = 0.0; m.t[2] = 0.0;
  if (row != nullptr) {
    m.t[0] = row[0]; m.t[1] = row[1]; m.t[2] = row[2];
    double w = row[3], x = row[4], y = row[5], z = row[6];
    const double nq = w * w + x * x + y * y + z * z;
    if (!(nq < 1e-8)) {
      const double inv = (w < 0.0 ? -1.0 : 1.0) / sqrt(nq);
      w *= inv; x *= inv; y *= inv; z *= inv;
      const double nv = sqrt(x * x + y * y + z * z);
      m.theta = 2.0 * atan2(nv, w);
      if (nv > 0.0) {
        m.k[0] = x / nv; m.k[1] = y / nv; m.k[2] = z / nv;
      }
    }
  }
  m.identity = m.theta == 0.0 && m.t[0] == 0.0 && m.t[1] == 0.0 && m.t[2] == 0.0;
  return m;
}

// The running minimum / maximum of the finite times a thread has seen.
struct DeskewRange {
  double lo, hi;        // +inf / -inf: none yet
};
__device__ __forceinline__ DeskewRange deskew_range_empty() { return DeskewRange{(double)INFINITY, -(double)INFINITY}; }
__device__ __forceinline__ void deskew_range_add(DeskewRange &r, double tau) {
  if (isfinite(tau)) {
    r.lo = fmin(r.lo, tau);
    r.hi = fmax(r.hi, tau);
  }
}
// All threads of a 1024-thread workgroup call this (it holds barriers): wave reduce, then 16 LDS slots -> the range of the
// whole workgroup in every thread.  lds: 32 doubles.  Minimum and maximum do not depend on the order of their operands.
__device__ __forceinline__ DeskewRange deskew_range_reduce(DeskewRange r, double *lds) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    r.lo = fmin(r.lo, __shfl_xor(r.lo, d, 64));
    r.hi = fmax(r.hi, __shfl_xor(r.hi, d, 64));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();                                       // an earlier use of lds has been read by everyone
  if (lane == 0) {
    lds[wave] = r.lo;
    lds[16 + wave] = r.hi;
  }
  __syncthreads();
  DeskewRange all = deskew_range_empty();
  for (int w = 0; w < 16; ++w) {
    all.lo = fmin(all.lo, lds[w]);
    all.hi = fmax(all.hi, lds[16 + w]);
  }
  return all;
}

// alpha of a kept row: 0 when the sweep has no time range (no finite time, or all equal) or the row's time is not finite.
__device__ __forceinline__ double deskew_alpha(double tau, const DeskewRange r) {
  if (!(r.hi > r.lo) || !isfinite(tau)) return 0.0;
  return (tau - r.lo) / (r.hi - r.lo);
}

// o = R(alpha) p + alpha t (Rodrigues' formula about the unit axis k), rounded to fp32 once; alpha == 0 or the identity
// motion: the bits of p.
__device__ __forceinline__ void deskew_row(const float p[3], double alpha, const DeskewMotion &m, float o[3]) {
  if (alpha == 0.0 || m.identity) {
    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
    return;
  }
  const double phi = alpha * m.theta;
  const double s = sin(phi), c = cos(phi);
  const double x = p[0], y = p[1], z = p[2];
  const double cx = m.k[1] * z - m.k[2] * y, cy = m.k[2] * x - m.k[0] * z, cz = m.k[0] * y - m.k[1] * x;      // k x p
  const double d = ((m.k[0] * x + m.k[1] * y) + m.k[2] * z) * (1.0 - c);
  o[0] = (float)(((x * c + cx * s) + m.k[0] * d) + alpha * m.t[0]);
  o[1] = (float)(((y * c + cy * s) + m.k[1] * d) + alpha * m.t[1]);
  o[2] = (float)(((z * c + cz * s) + m.k[2] * d) + alpha * m.t[2]);
}

}  // namespace pwclo
