// Arithmetic of the point-to-plane registration against a sliding local map, shared by the kernels of
// icp.hip, projective.hip and voxel_map.hip and by host code that wants the same numbers: one definition of a normal, of a
// row of the normal equations, of the 6x6 solve and of the pose update (the pattern of grid.hpp, deskew.hpp and rows.hpp),
// and the two pieces the three refiners' kernels have in common: the end of an accumulate kernel (icp_reduce_store_row,
// icp_store_zero_row) and what a map slot does after a push (icp_slot_after_push).  Everything here is fp64 on fp32 inputs;
// no function has a data-dependent loop bound.
//
// Conventions.  A pose is an Se3 (se3.hpp, which holds all rigid-transform arithmetic).  The registered pose T of a frame
// maps that frame's points into the previous frame.  A twist is [w, v], rotation first, and updates from the left:
// T <- [Rodrigues(w) | v] T.
#pragma once
#include <math.h>

#include "common.hpp"
#include "se3.hpp"

namespace pwclo {

#define ICP_HD __host__ __device__ static inline

// One row of sums: 21 upper entries of sum w^2 J^T J (row-major, i <= j), 6 of sum w^2 J r, sum w^2, sum w^2 r^2, pairs,
// two words of padding (a row is 256 bytes).
constexpr int ICP_ROW = 32;
constexpr int ICP_H = 0, ICP_G = 21, ICP_SW = 27, ICP_COST = 28, ICP_PAIRS = 29, ICP_TERMS = 30;
// Why a stream froze (status word; 0: still moving).
constexpr int ICP_CONVERGED = 1, ICP_FEW_PAIRS = 2, ICP_BAD_PIVOT = 4;
constexpr int ICP_IDLE = 8;                 // masked registration: the stream delivered no frame in this call
constexpr int ICP_JACOBI_SWEEPS = 8;        // cyclic Jacobi on a symmetric 3x3 converges quadratically: 8 sweeps is past fp64
// The rank test of a normal: with l_min <= l_mid <= l_max the eigenvalues of the neighbourhood's covariance, the rank is
// below 2 (duplicates: l_max = 0; collinear neighbours: l_mid = 0 up to rounding) iff !(l_mid > ICP_RANK_EPS * l_max).
// Products of fp32 coordinates are exact in fp64, so an exactly collinear neighbourhood gives l_mid / l_max ~ 1e-16, and a
// neighbourhood whose second extent is above sqrt(1e-10) = 1e-5 of its first passes.  NaN fails the test.
constexpr double ICP_RANK_EPS = 1e-10;
constexpr double ICP_HUBER_CLAMP = 1e-4;    // the reference's _WLSScheme.eps
constexpr int ICP_ACC_THREADS = 256;        // points per workgroup of the accumulation = per partial row

// ---- normals -----------------------------------------------------------------------------------------------------------------

// Eigen-decomposition of the symmetric 3x3 matrix c = [xx xy xz yy yz zz]: val ascending, vec the unit eigenvector of val[0].
// A NaN off the diagonal is skipped like a zero (no rotation can remove it), so the diagonal then decides alone; the
// covariance of a neighbourhood with a NaN or Inf point has a diagonal that is not finite either, and icp_normal's rank test
// turns that into the zero normal.
ICP_HD void icp_eig3(const double c[6], double val[3], double vec[3]) {
  double a[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}};
  double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
#pragma unroll 1
  for (int sweep = 0; sweep < ICP_JACOBI_SWEEPS; ++sweep) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int p = r == 2 ? 1 : 0, q = r == 0 ? 1 : 2;                    // (0,1), (0,2), (1,2)
      const double apq = a[p][q];
      if (apq == 0.0 || apq != apq) continue;
      const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
      const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));   // |theta| = inf: t = 0
      const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
      const int o = 3 - p - q;
      const double app = a[p][p], aqq = a[q][q], aop = a[o][p], aoq = a[o][q];
      a[p][p] = app - t * apq;
      a[q][q] = aqq + t * apq;
      a[p][q] = 0.0; a[q][p] = 0.0;
      a[o][p] = cs * aop - sn * aoq; a[p][o] = a[o][p];
      a[o][q] = sn * aop + cs * aoq; a[q][o] = a[o][q];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double vip = v[i][p], viq = v[i][q];
        v[i][p] = cs * vip - sn * viq;
        v[i][q] = sn * vip + cs * viq;
      }
    }
  }
  const double d0 = a[0][0], d1 = a[1][1], d2 = a[2][2];
  const int lo = (d0 <= d1 && d0 <= d2) ? 0 : (d1 <= d2 ? 1 : 2);
  const double e1 = lo == 0 ? d1 : d0, e2 = lo == 2 ? d1 : d2;             // the other two
  val[0] = lo == 0 ? d0 : (lo == 1 ? d1 : d2);
  val[1] = e1 <= e2 ? e1 : e2;
  val[2] = e1 <= e2 ? e2 : e1;
  const double x = lo == 0 ? v[0][0] : (lo == 1 ? v[0][1] : v[0][2]);
  const double y = lo == 0 ? v[1][0] : (lo == 1 ? v[1][1] : v[1][2]);
  const double z = lo == 0 ? v[2][0] : (lo == 1 ? v[2][1] : v[2][2]);
  const double inv = 1.0 / sqrt((x * x + y * y) + z * z);
  vec[0] = x * inv; vec[1] = y * inv; vec[2] = z * inv;
}

// The normal of a point y from the covariance c of (neighbour - y): the unit eigenvector of the smallest eigenvalue turned
// towards the origin (n . y <= 0), rounded to fp32; the zero vector where the rank test above fails.  eig: ascending.
ICP_HD void icp_normal(const double c[6], const float y[3], float out[3], double eig[3]) {
  double vec[3];
  icp_eig3(c, eig, vec);
  if (!(eig[1] > ICP_RANK_EPS * eig[2])) {
    out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f;
    return;
  }
  const double d = (vec[0] * (double)y[0] + vec[1] * (double)y[1]) + vec[2] * (double)y[2];
  const double sg = d > 0.0 ? -1.0 : 1.0;
  out[0] = (float)(sg * vec[0]); out[1] = (float)(sg * vec[1]); out[2] = (float)(sg * vec[2]);
}

// ---- one row of the normal equations -------------------------------------------------------------------------------------------

// The reference's _HuberScheme through _WLSScheme.weights, squared: cost / max(|r|, eps)^2 with cost = r^2 below sigma.
ICP_HD double icp_huber_w2(double r, double sigma) {
  const double ar = fabs(r);
  if (ar < sigma) return 1.0;
  const double cl = ar > ICP_HUBER_CLAMP ? ar : ICP_HUBER_CLAMP;
  return (2.0 * sigma * ar - sigma * sigma) / (cl * cl);
}

// Adds the pair (query q matched to map point y with normal n, both in slot coordinates, all fp32 values) to acc.  p: the
// frame's point, T: its pose estimate, Rm: the 3x3 rotation from the slot into the previous frame.
ICP_HD void icp_add_pair(const float p[3], const float q[3], const float y[3], const float n[3], const Se3 &T,
                         const double Rm[9], double sigma, double acc[ICP_TERMS]) {
  const double r = (((double)n[0] * ((double)q[0] - (double)y[0])) + ((double)n[1] * ((double)q[1] - (double)y[1]))) +
                   ((double)n[2] * ((double)q[2] - (double)y[2]));
  double np[3], pp[3], J[6];
#pragma unroll
  for (int i = 0; i < 3; ++i) np[i] = (Rm[3 * i] * (double)n[0] + Rm[3 * i + 1] * (double)n[1]) + Rm[3 * i + 2] * (double)n[2];
  se3_apply(T, p, pp);
  J[0] = pp[1] * np[2] - pp[2] * np[1];
  J[1] = pp[2] * np[0] - pp[0] * np[2];
  J[2] = pp[0] * np[1] - pp[1] * np[0];
  J[3] = np[0]; J[4] = np[1]; J[5] = np[2];
  const double w2 = icp_huber_w2(r, sigma);
  int e = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double wj = w2 * J[i];
#pragma unroll
    for (int j = i; j < 6; ++j) acc[ICP_H + e++] += wj * J[j];
    acc[ICP_G + i] += wj * r;
  }
  acc[ICP_SW] += w2;
  acc[ICP_COST] += w2 * (r * r);
  acc[ICP_PAIRS] += 1.0;
}

// ---- solve and update ------------------------------------------------------------------------------------------------------------

// delta = -(H / sw + damping I)^-1 (g / sw) from a row of sums, by Cholesky.  false (delta untouched) when a pivot is not
// positive (NaN included) or the step is not finite: a NaN in g alone passes every pivot, and would otherwise reach the pose.
ICP_HD bool icp_solve6(const double sum[ICP_ROW], double damping, double delta[6]) {
  double L[6][6], b[6];
  const double sw = sum[ICP_SW];
  int e = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = i; j < 6; ++j) {
      const double h = sum[ICP_H + e++] / sw;
      L[j][i] = i == j ? h + damping : h;              // the lower triangle, to be factored in place
    }
    b[i] = sum[ICP_G + i] / sw;
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = L[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    if (!(d > 0.0)) ok = false;
    const double piv = sqrt(d);
    L[j][j] = piv;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double s = L[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      L[i][j] = s / piv;
    }
  }
  if (!ok) return false;
#pragma unroll
  for (int i = 0; i < 6; ++i) {                        // L z = b
    double s = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= L[i][k] * b[k];
    b[i] = s / L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {                       // L^T x = z
    double s = b[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s -= L[k][i] * b[k];
    b[i] = s / L[i][i];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i)
    if (!(fabs(b[i]) <= 1.7976931348623157e308)) return false;   // NaN or inf
#pragma unroll
  for (int i = 0; i < 6; ++i) delta[i] = -b[i];
  return true;
}

// T <- [Rodrigues(w) | v] T, then the rotation re-orthonormalised by Gram-Schmidt on its columns (first column kept in
// direction, third = first x second).  Rodrigues: I + a K + b K^2, a = sin(th) / th, b = (sin(th / 2) / (th / 2))^2 / 2.
ICP_HD void icp_update_pose(const double delta[6], Se3 &T) {
  const double wx = delta[0], wy = delta[1], wz = delta[2];
  const double th2 = (wx * wx + wy * wy) + wz * wz, th = sqrt(th2);
  double a = 1.0, b = 0.5;
  if (th > 0.0) {
    const double h = sin(0.5 * th) / (0.5 * th);
    a = sin(th) / th;
    b = 0.5 * (h * h);
  }
  Se3 E;
  E.m[0] = 1.0 - b * (wy * wy + wz * wz); E.m[1] = b * (wx * wy) - a * wz;        E.m[2] = b * (wx * wz) + a * wy;
  E.m[4] = b * (wx * wy) + a * wz;        E.m[5] = 1.0 - b * (wx * wx + wz * wz); E.m[6] = b * (wy * wz) - a * wx;
  E.m[8] = b * (wx * wz) - a * wy;        E.m[9] = b * (wy * wz) + a * wx;        E.m[10] = 1.0 - b * (wx * wx + wy * wy);
  E.m[3] = delta[3]; E.m[7] = delta[4]; E.m[11] = delta[5];
  const Se3 N = se3_mul(E, T);
  double c0[3] = {N.m[0], N.m[4], N.m[8]}, c1[3] = {N.m[1], N.m[5], N.m[9]};
  const double i0 = 1.0 / sqrt((c0[0] * c0[0] + c0[1] * c0[1]) + c0[2] * c0[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i) c0[i] *= i0;
  const double d = (c0[0] * c1[0] + c0[1] * c1[1]) + c0[2] * c1[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) c1[i] -= d * c0[i];
  const double i1 = 1.0 / sqrt((c1[0] * c1[0] + c1[1] * c1[1]) + c1[2] * c1[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i) c1[i] *= i1;
  const double c2[3] = {c0[1] * c1[2] - c0[2] * c1[1], c0[2] * c1[0] - c0[0] * c1[2], c0[0] * c1[1] - c0[1] * c1[0]};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    T.m[4 * i] = c0[i]; T.m[4 * i + 1] = c1[i]; T.m[4 * i + 2] = c2[i]; T.m[4 * i + 3] = N.m[4 * i + 3];
  }
}

// ---- what the refiners' kernels share ------------------------------------------------------------------------------------------

// The end of an accumulate kernel (a workgroup of ICP_ACC_THREADS, every thread arrives): the threads' acc -> the
// workgroup's row of partial (S, gridDim.x, ICP_ROW), s = the workgroup's stream.  Every term goes through the xor butterfly
// of its wave (32, 16, .., 1), then the four waves' results are added in the order 0, 1, 2, 3; the two padding words are
// zero.  The order is fixed so that two runs, and the three refiners on the same pairs, give the same bits; it is the
// parity contract with tests/icp_model.py, whose accumulate() adds the same terms and allows for this order of adding
// them by the rounding of the sum of their magnitudes.  Change it here, for all three kernels at once, or not at all.
__device__ __forceinline__ void icp_reduce_store_row(const double acc[ICP_TERMS], double *__restrict__ partial, int s) {
  __shared__ double wave_row[ICP_ACC_THREADS / 64][ICP_ROW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int e = 0; e < ICP_TERMS; ++e) {
    double v = acc[e];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    if (lane == 0) wave_row[wave][e] = v;
  }
  __syncthreads();
  if (threadIdx.x < ICP_ROW) {
    double v = 0.0;
    if (threadIdx.x < ICP_TERMS) {
      v = wave_row[0][threadIdx.x];
#pragma unroll
      for (int w = 1; w < ICP_ACC_THREADS / 64; ++w) v += wave_row[w][threadIdx.x];
    }
    partial[((size_t)s * gridDim.x + blockIdx.x) * ICP_ROW + threadIdx.x] = v;
  }
}
// The row of an idle stream's workgroup: zeros, nothing gathered.  The whole workgroup leaves after it.
__device__ __forceinline__ void icp_store_zero_row(double *__restrict__ partial, int s) {
  if (threadIdx.x < ICP_ROW) partial[((size_t)s * gridDim.x + blockIdx.x) * ICP_ROW + threadIdx.x] = 0.0;
}

// A map slot emptied or just filled: A = I (all 16 words) and, where the refiner keeps one (Rm != nullptr), Rm = I.
__device__ __forceinline__ void icp_slot_identity(double *A, double *Rm) {
  se3_store(A, se3_identity());
  if (Rm != nullptr) {
#pragma unroll
    for (int e = 0; e < 9; ++e) Rm[e] = (e % 4 == 0) ? 1.0 : 0.0;
  }
}
// What one slot does after a push of the frame with pose T (4x4): the slot the frame went to (fresh) becomes the identity
// and live; any other live slot is re-based on the new frame, A <- A T in rows 0..2 (row 3 stays) and Rm <- R_T^T Rm.  The
// caller moves the cursor, after a barrier.
__device__ __forceinline__ void icp_slot_after_push(bool fresh, int *live, double *A, const double *T, double *Rm) {
  if (fresh) {
    icp_slot_identity(A, Rm);
    *live = 1;
  } else if (*live != 0) {
    const Se3 t = se3_load(T);
    se3_store_rows(A, se3_mul(se3_load(A), t));
    if (Rm != nullptr) {
      double r[9];
#pragma unroll
      for (int e = 0; e < 9; ++e) r[e] = Rm[e];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Rm[3 * i + j] = (t.m[i] * r[j] + t.m[4 + i] * r[3 + j]) + t.m[8 + i] * r[6 + j];
    }
  }
}

}  // namespace pwclo
