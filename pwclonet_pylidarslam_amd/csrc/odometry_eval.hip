// KITTI odometry evaluation of predicted poses on the device (gfx950).
//
// The reference turns every batch's pose rows into 4x4 matrices on the HOST, one sample at a time
// (train.py:866-893: D2H copy, quat2mat, np.linalg.inv per sample), chains them with a Python loop
// (kitti360_utils.py:406-431), writes text files and re-reads them to compute the KITTI segment errors with
// three nested Python loops (evaluation.py:236-271 / slam/eval/eval_odometry.py:316-361).  Here the pose rows
// stay in HBM as the network wrote them; four small fp64 kernels do the rest for ALL sequences at once:
//   rows -> transforms        one thread per frame                      (train.py:762-795 quat2mat, :873-878)
//   transforms -> trajectory  one wave per sequence, chunked scan       (kitti360_utils.py:422-426)
//   trajectory -> distances   one wave per sequence, chunked scan       (evaluation.py:198-215)
//   segment errors            one thread per (first frame, length)      (evaluation.py:236-271)
// The work is a few thousand 4x4 fp64 products: latency-bound, nowhere near any roofline; the point is that
// nothing leaves the device and no host loop runs per frame.  SE(3) composition is associative, so the scans
// differ from the reference's sequential products only by fp64 rounding (tests: 1e-9).
#include "common.hpp"
#include "se3.hpp"

namespace pwclo {

__global__ __launch_bounds__(256) void odom_rows_to_transforms_kernel(int n, int row_stride,
                                                                      const float *__restrict__ rows,
                                                                      double *__restrict__ T, int invert) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  Se3 a = pose_row_to_se3(rows + (size_t)i * row_stride);
  if (invert) a = se3_inv(a);
  se3_store(T + (size_t)i * 16, a);
}

// abs[f] = T[0] . T[1] ... T[f] within each sequence (kitti360_utils.py:422-426 with rel = T^-1:
// abs[f] = inv(rel[f] @ inv(abs[f-1])) = abs[f-1] . T[f], abs[-1] = I).  One wave per sequence: every lane
// multiplies a contiguous chunk, the 64 chunk products are scanned with 6 shuffle steps, then each lane
// replays its chunk from its exclusive prefix.
__global__ __launch_bounds__(64) void odom_accumulate_kernel(const int *__restrict__ seq_start,
                                                             const double *__restrict__ T,
                                                             double *__restrict__ abs_out) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const int lo = seq_start[s], n = seq_start[s + 1] - lo;
  if (n <= 0) return;
  const int chunk = (n + 63) / 64;
  const int c0 = min(lane * chunk, n), c1 = min(c0 + chunk, n);
  Se3 prod = se3_identity();
  for (int i = c0; i < c1; ++i) prod = se3_mul(prod, se3_load(T + (size_t)(lo + i) * 16));
  Se3 incl = prod;                                   // inclusive scan over lanes (left operand = earlier lanes)
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const Se3 up = se3_shfl_up(incl, d);
    if (lane >= d) incl = se3_mul(up, incl);
  }
  Se3 run = se3_shfl_up(incl, 1);                    // exclusive prefix
  if (lane == 0) run = se3_identity();
  for (int i = c0; i < c1; ++i) {
    run = se3_mul(run, se3_load(T + (size_t)(lo + i) * 16));
    se3_store(abs_out + (size_t)(lo + i) * 16, run);
  }
}

// evaluation.py:198-215 / eval_odometry.py:268-276: dist[0] = 0, dist[i] = dist[i-1] + |p[i] - p[i-1]|.
__global__ __launch_bounds__(64) void odom_cumdist_kernel(const int *__restrict__ seq_start,
                                                          const double *__restrict__ poses,
                                                          double *__restrict__ dist) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const int lo = seq_start[s], n = seq_start[s + 1] - lo;
  if (n <= 0) return;
  const int chunk = (n + 63) / 64;
  const int c0 = min(lane * chunk, n), c1 = min(c0 + chunk, n);
  auto step = [&](int i) -> double {                 // length of the move INTO frame i (0 for the first frame)
    if (i == 0) return 0.0;
    const double *a = poses + (size_t)(lo + i - 1) * 16, *b = poses + (size_t)(lo + i) * 16;
    const double dx = a[3] - b[3], dy = a[7] - b[7], dz = a[11] - b[11];
    return sqrt(dx * dx + dy * dy + dz * dz);
  };
  double sum = 0.0;
  for (int i = c0; i < c1; ++i) sum += step(i);
  double incl = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double up = f64_shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  double run = f64_shfl_up(incl, 1);
  if (lane == 0) run = 0.0;
  for (int i = c0; i < c1; ++i) {
    run += step(i);
    dist[lo + i] = run;
  }
}

// evaluation.py:236-271 (= eval_odometry.py:316-361): for every first frame f = 0, step, 2*step, ... and every
// segment length L: last = first i >= f with dist[i] > dist[f] + L.  The reference searches linearly; this is an
// upper-bound search, the same frame wherever dist is non-decreasing.  odom_cumdist_kernel's dist is that only up to an
// ulp: over a stationary stretch a lane's prefix may sit one ulp below the previous lane's last value, so the two
// searches can part only if dist[f] + L falls inside such an ulp, and then by frames of one pose (DESIGN.md section 8,
// f4).  pose_error = inv(inv(R[f]) R[last]) . (inv(G[f]) G[last]);
// row = [f, r_err / L, t_err / L, L, speed], speed = L / (0.1 * (last - f + 1)).
__global__ __launch_bounds__(256) void odom_sequence_errors_kernel(int nseq, const int *__restrict__ seq_start,
                                                                   const int *__restrict__ slot_start,
                                                                   const double *__restrict__ gt,
                                                                   const double *__restrict__ res,
                                                                   const double *__restrict__ dist, int step,
                                                                   int nlen, const double *__restrict__ lengths,
                                                                   double *__restrict__ err,
                                                                   int *__restrict__ valid) {
  const int slot = blockIdx.x * 256 + threadIdx.x;
  if (slot >= slot_start[nseq]) return;
  int s = 0;                                          // few sequences: linear search for the owner
  while (s + 1 < nseq && slot >= slot_start[s + 1]) ++s;
  const int local = slot - slot_start[s];
  const int lo = seq_start[s], n = seq_start[s + 1] - lo;
  const int first = (local / nlen) * step, li = local % nlen;
  const double L = lengths[li];
  const double *d = dist + lo;
  const double target = d[first] + L;
  int a = first, b = n;                               // first index in [first, n) with d[i] > target
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (d[mid] > target) b = mid; else a = mid + 1;
  }
  double *row = err + (size_t)slot * 5;
  if (a >= n) {
    valid[slot] = 0;
    row[0] = first; row[1] = 0.0; row[2] = 0.0; row[3] = L; row[4] = 0.0;
    return;
  }
  const int last = a;
  const Se3 dg = se3_mul(se3_inv(se3_load(gt + (size_t)(lo + first) * 16)), se3_load(gt + (size_t)(lo + last) * 16));
  const Se3 dr = se3_mul(se3_inv(se3_load(res + (size_t)(lo + first) * 16)), se3_load(res + (size_t)(lo + last) * 16));
  const Se3 e = se3_mul(se3_inv(dr), dg);
  const double tr = 0.5 * (e.m[0] + e.m[5] + e.m[10] - 1.0);
  const double r_err = acos(fmax(fmin(tr, 1.0), -1.0));
  const double t_err = sqrt(e.m[3] * e.m[3] + e.m[7] * e.m[7] + e.m[11] * e.m[11]);
  const double frames = (double)(last - first) + 1.0;
  valid[slot] = 1;
  row[0] = first; row[1] = r_err / L; row[2] = t_err / L; row[3] = L; row[4] = L / (0.1 * frames);
}

}  // namespace pwclo

using namespace pwclo;

extern "C" void odom_rows_to_transforms_kernel_wrapper(int n, int row_stride, const float *rows, double *T,
                                                       int invert) {
  if (n <= 0) return;
  PWCLO_REQUIRE(row_stride >= 7, "odom_rows_to_transforms: row_stride=%d must be >= 7", row_stride);
  hipLaunchKernelGGL(odom_rows_to_transforms_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, current_stream(), n,
                     row_stride, rows, T, invert);
  check_launch("odom_rows_to_transforms");
}

extern "C" void odom_accumulate_kernel_wrapper(int nseq, const int *seq_start, const double *T, double *abs_out) {
  if (nseq <= 0) return;
  hipLaunchKernelGGL(odom_accumulate_kernel, dim3(nseq), dim3(64), 0, current_stream(), seq_start, T, abs_out);
  check_launch("odom_accumulate");
}

extern "C" void odom_cumulative_distance_kernel_wrapper(int nseq, const int *seq_start, const double *poses,
                                                        double *dist) {
  if (nseq <= 0) return;
  hipLaunchKernelGGL(odom_cumdist_kernel, dim3(nseq), dim3(64), 0, current_stream(), seq_start, poses, dist);
  check_launch("odom_cumulative_distance");
}

extern "C" void odom_sequence_errors_kernel_wrapper(int nseq, int total_slots, const int *seq_start,
                                                    const int *slot_start, const double *poses_gt,
                                                    const double *poses_result, const double *dist, int step,
                                                    int nlen, const double *lengths, double *err, int *valid) {
  if (nseq <= 0 || total_slots <= 0) return;
  PWCLO_REQUIRE(step >= 1 && nlen >= 1, "odom_sequence_errors: step=%d nlen=%d must be >= 1", step, nlen);
  hipLaunchKernelGGL(odom_sequence_errors_kernel, dim3(ceil_div(total_slots, 256)), dim3(256), 0, current_stream(),
                     nseq, seq_start, slot_start, poses_gt, poses_result, dist, step, nlen, lengths, err, valid);
  check_launch("odom_sequence_errors");
}
