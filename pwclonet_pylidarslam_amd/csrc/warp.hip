// Quaternion pose warp for gfx950.  Replaces PW/PWCLO_utils.py:31-63 (warp = two Hamilton
// products built from ~40 tiny torch ops, plus two host-side tensor constructions and H2D copies
// per call).  One thread per point, streaming (B,3,N) -> (B,3,N); the products follow the
// reference's term order (PWCLO_utils.py:83-95,117-129) without contraction so the warped
// coordinates -- which feed the neighbour searches of the refinement levels -- agree with the
// reference to the last bit wherever torch's own evaluation order is defined.
#include <stdint.h>

#include "common.hpp"
#include "rows.hpp"

PWCLO_TRACE_TU(warp)

namespace pwclo {

struct quat { float w, x, y, z; };

// Hamilton product a (x) b with the reference's left-to-right evaluation of each component.
__device__ __forceinline__ quat hamilton(const quat a, const quat b) {
  quat r;
  r.w = ((a.w * b.w - a.x * b.x) - a.y * b.y) - a.z * b.z;
  r.x = ((a.w * b.x + a.x * b.w) + a.y * b.z) - a.z * b.y;
  r.y = ((a.w * b.y - a.x * b.z) + a.y * b.w) + a.z * b.x;
  r.z = ((a.w * b.z + a.x * b.y) - a.y * b.x) + a.z * b.w;
  return r;
}

template <bool POINT_MAJOR>
__global__ __launch_bounds__(256) void quat_warp_kernel(int n, const float *__restrict__ xyz,
                                                        const float *__restrict__ q,
                                                        const float *__restrict__ t,
                                                        float *__restrict__ out) {
  TraceScope trace_scope_(TK_WARP);
  const int b = blockIdx.y;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const quat qq = {q[b * 4 + 0], q[b * 4 + 1], q[b * 4 + 2], q[b * 4 + 3]};
  // inv_q (PWCLO_utils.py:31-39): conj(q) / (sum(q*q) + 1e-10)
  const float q2 = (((qq.w * qq.w + qq.x * qq.x) + qq.y * qq.y) + qq.z * qq.z) + 1e-10f;
  const quat qi = {qq.w / q2, (qq.x * -1.0f) / q2, (qq.y * -1.0f) / q2, (qq.z * -1.0f) / q2};
  const float *src = xyz + (size_t)b * 3 * n;
  const int sx = POINT_MAJOR ? 3 * j : j, st = POINT_MAJOR ? 1 : n;  // (b,n,3) or (b,3,n)
  const quat p = {0.0f, src[sx], src[sx + st], src[sx + 2 * st]};
  const quat r = hamilton(hamilton(qq, p), qi);
  float *dst = out + (size_t)b * 3 * n;
  dst[sx] = r.x + t[b * 3 + 0];
  dst[sx + st] = r.y + t[b * 3 + 1];
  dst[sx + 2 * st] = r.z + t[b * 3 + 2];
}

// Input adapter of the fused pipeline: two (B,3,N) channel-major clouds (what PWCLONet.forward
// receives, pwclo_net.py:125-126) -> one point-major (2B,N,3) batch (frame 1 first).  Replaces
// torch.cat + permute + contiguous (three passes) by one.
__global__ __launch_bounds__(256) void ingest_pairs_kernel(int bsz, int n, const float *__restrict__ f1,
                                                           const float *__restrict__ f2,
                                                           float *__restrict__ out) {
  TraceScope trace_scope_(TK_INGEST, 15u);
  const int b = blockIdx.y;               // 0 .. 2*bsz-1
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const float *src = (b < bsz ? f1 + (size_t)b * 3 * n : f2 + (size_t)(b - bsz) * 3 * n);
  float *dst = out + ((size_t)b * n + j) * 3;
  dst[0] = src[j];
  dst[1] = src[n + j];
  dst[2] = src[2 * n + j];
}

// Input adapter one level up (prediction_modules.py:144-160): two point-major frames (B, n_total, c),
// c >= 3 floats per point, of which the first n points and the first 3 channels are used
// (`pcd[:, :num_points, :3]`) -> the same (2B,n,3) batch.  Replaces slice + permute + contiguous in
// the reference's adapter and the permute back in the fused forward.
// Point j of output cloud b: the first 3 of the c floats of `frame`'s row j.
__device__ __forceinline__ void ingest_point(int b, int j, int n, int c, const float *__restrict__ frame,
                                             float *__restrict__ out) {
  const float *src = frame + (size_t)j * c;
  float *dst = out + ((size_t)b * n + j) * 3;
  dst[0] = src[0];
  dst[1] = src[1];
  dst[2] = src[2];
}

__global__ __launch_bounds__(256) void ingest_frames_kernel(int bsz, int n, int n_total, int c,
                                                            const float *__restrict__ f1,
                                                            const float *__restrict__ f2,
                                                            float *__restrict__ out) {
  const int b = blockIdx.y;               // 0 .. 2*bsz-1
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  ingest_point(b, j, n, c, b < bsz ? f1 + (size_t)b * n_total * c : f2 + (size_t)(b - bsz) * n_total * c, out);
}

// Sequence form (FusedPWCLONet.sample_sequence): one window of t frames (t, n_total, c) -> (t, n, 3), frame order kept;
// every frame is ingested once and serves as frame 2 of one pair and frame 1 of the next.
__global__ __launch_bounds__(256) void ingest_sequence_kernel(int n, int n_total, int c, const float *__restrict__ frames,
                                                              float *__restrict__ out) {
  const int b = blockIdx.y;               // 0 .. t-1
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  ingest_point(b, j, n, c, frames + (size_t)b * n_total * c, out);
}

// The row bodies of the raw-frame filters (kitti_row, kitti360_row) live in rows.hpp, shared with train_batch.hip.

// One thread per point; HBM-trivial (16 bytes in, 16 bytes out per point).
__global__ __launch_bounds__(256) void kitti_transform_filter_kernel(int n, const double *__restrict__ tr,
                                                                     const float *__restrict__ points,
                                                                     float *__restrict__ xyz,
                                                                     int *__restrict__ keep) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 p = *reinterpret_cast<const float4 *>(points + (size_t)i * 4);   // (x, y, z, intensity)
  float o[3];
  const bool k = kitti_row(p, tr, o);
  xyz[(size_t)i * 3 + 0] = o[0];
  xyz[(size_t)i * 3 + 1] = o[1];
  xyz[(size_t)i * 3 + 2] = o[2];
  keep[i] = k ? 1 : 0;
}

__global__ __launch_bounds__(256) void kitti360_filter_kernel(int n, float ground_z, float near,
                                                              const float *__restrict__ points,
                                                              float *__restrict__ xyz, int *__restrict__ keep) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 p = *reinterpret_cast<const float4 *>(points + (size_t)i * 4);
  float o[3];
  const bool k = kitti360_row(p, ground_z, near, o);
  xyz[(size_t)i * 3 + 0] = o[0];
  xyz[(size_t)i * 3 + 1] = o[1];
  xyz[(size_t)i * 3 + 2] = o[2];
  keep[i] = k ? 1 : 0;
}

// Stable per-frame compaction of the kept rows (keep != 0): kept row number p (frame order, from 0) of frame f goes to
// out[f, p]; rows >= count stay as the caller zero-filled them (the sampler never selects zero rows).  Rows beyond `cap`
// are dropped (the caller sizes cap >= max count).  The scan is inside the kernel (it used to be torch.cumsum, a library
// kernel on the product path of BASELINE configs[4]): one 1024-thread workgroup per frame; wave w owns a contiguous range
// of rows and walks it 64 rows at a time (coalesced), a ballot + popcount gives every kept row its slot inside the step,
// the running sum of popcounts its slot inside the wave's range; the 16 waves' totals are scanned through LDS between a
// counting pass and the writing pass.  Stable (frame order).
__global__ __launch_bounds__(1024) void compact_frames_scan_kernel(int n, int cap, const int *__restrict__ keep,
                                                                   const float *__restrict__ xyz,
                                                                   float *__restrict__ out, int *__restrict__ counts) {
  __shared__ int wave_total[16];
  const int f = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per_wave = ((n + 15) / 16 + 63) / 64 * 64;          // multiple of 64: steps never straddle two waves' ranges
  const int i0 = wave * per_wave, i1 = min(n, i0 + per_wave);
  const int *kf = keep + (size_t)f * n;
  int total = 0;
  for (int i = i0 + lane; i - lane < i1; i += 64)
    total += __popcll(__ballot(i < i1 && kf[i] != 0));
  if (lane == 0) wave_total[wave] = total;
  __syncthreads();
  int base = 0, all = 0;
  for (int w = 0; w < 16; ++w) {
    const int t = wave_total[w];
    if (w < wave) base += t;
    all += t;
  }
  const float *xf = xyz + (size_t)f * n * 3;
  float *of = out + (size_t)f * cap * 3;
  for (int i = i0 + lane; i - lane < i1; i += 64) {
    const bool k = i < i1 && kf[i] != 0;
    const unsigned long long m = __ballot(k);
    const int p = base + mbcnt64(m);
    if (k && p < cap) {
      of[(size_t)p * 3 + 0] = xf[(size_t)i * 3 + 0];
      of[(size_t)p * 3 + 1] = xf[(size_t)i * 3 + 1];
      of[(size_t)p * 3 + 2] = xf[(size_t)i * 3 + 2];
    }
    base += __popcll(m);
  }
  if (threadIdx.x == 0) counts[f] = all < cap ? all : cap;
}

// Raw sweeps of S streams, each of its own length, -> packed survivors in ONE launch (StreamingOdometry.step_sweeps,
// DESIGN.md section 12): the filters' row bodies above + compact_frames_scan_kernel's layout (one 1024-thread workgroup
// per stream, ballot / popcount counting pass, LDS scan of the 16 wave totals, writing pass; the row is evaluated again
// in the writing pass rather than kept: 16 bytes per row, HBM-trivial next to the sampler).  The length is read from
// device memory and only rows [0, length) of the stream are touched, so one captured graph serves every length up to R.
// The kernel also zeroes rows [count, cap) of its output: a persistent buffer never shows the previous sweep's survivors.
template <bool KITTI>
__global__ __launch_bounds__(1024) void sweep_filter_compact_kernel(int R, int cap, const int *__restrict__ lengths,
                                                                    const float *__restrict__ sweeps,
                                                                    const double *__restrict__ tr, float ground_z,
                                                                    float near, float *__restrict__ packed,
                                                                    int *__restrict__ counts) {
  __shared__ int wave_total[16];
  const int s = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = min(max(lengths[s], 0), R);
  const int per_wave = ((n + 15) / 16 + 63) / 64 * 64;          // multiple of 64: steps never straddle two waves' ranges
  const int i0 = wave * per_wave, i1 = min(n, i0 + per_wave);
  const float *sf = sweeps + (size_t)s * R * 4;
  const double *ts = KITTI ? tr + (size_t)s * 12 : nullptr;
  auto row = [&](int i, float o[3]) {
    const float4 p = *reinterpret_cast<const float4 *>(sf + (size_t)i * 4);
    return KITTI ? kitti_row(p, ts, o) : kitti360_row(p, ground_z, near, o);
  };
  int total = 0;
  for (int i = i0 + lane; i - lane < i1; i += 64) {
    float o[3];
    total += __popcll(__ballot(i < i1 && row(i, o)));
  }
  if (lane == 0) wave_total[wave] = total;
  __syncthreads();
  int base = 0, all = 0;
  for (int w = 0; w < 16; ++w) {
    const int t = wave_total[w];
    if (w < wave) base += t;
    all += t;
  }
  float *of = packed + (size_t)s * cap * 3;
  for (int i = i0 + lane; i - lane < i1; i += 64) {
    float o[3];
    const bool k = i < i1 && row(i, o);
    const unsigned long long m = __ballot(k);
    const int p = base + mbcnt64(m);
    if (k && p < cap) {
      of[(size_t)p * 3 + 0] = o[0];
      of[(size_t)p * 3 + 1] = o[1];
      of[(size_t)p * 3 + 2] = o[2];
    }
    base += __popcll(m);
  }
  const int count = all < cap ? all : cap;
  for (size_t j = (size_t)count * 3 + threadIdx.x; j < (size_t)cap * 3; j += 1024) of[j] = 0.0f;   // disjoint from the survivors
  if (threadIdx.x == 0) counts[s] = count;
}

}  // namespace pwclo

using namespace pwclo;

extern "C" void kitti_transform_filter_kernel_wrapper(int n, const double *tr, const float *points, float *xyz,
                                                      int *keep) {
  if (n <= 0) return;
  PWCLO_REQUIRE((reinterpret_cast<uintptr_t>(points) & 15) == 0, "kitti_transform_filter: points must be 16-byte aligned%s", "");
  hipLaunchKernelGGL(kitti_transform_filter_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, current_stream(), n, tr,
                     points, xyz, keep);
  check_launch("kitti_transform_filter");
}

extern "C" void kitti360_filter_kernel_wrapper(int n, float ground_z, float near, const float *points, float *xyz,
                                               int *keep) {
  if (n <= 0) return;
  PWCLO_REQUIRE((reinterpret_cast<uintptr_t>(points) & 15) == 0, "kitti360_filter: points must be 16-byte aligned%s", "");
  hipLaunchKernelGGL(kitti360_filter_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, current_stream(), n, ground_z,
                     near, points, xyz, keep);
  check_launch("kitti360_filter");
}

extern "C" void compact_frames_scan_kernel_wrapper(int b, int n, int cap, const int *keep, const float *xyz, float *out,
                                                   int *counts) {
  if (b <= 0 || n <= 0) return;
  PWCLO_REQUIRE(cap > 0 && (long long)n * 3 < (1ll << 31), "compact_frames_scan: n=%d cap=%d out of range", n, cap);
  hipLaunchKernelGGL(compact_frames_scan_kernel, dim3(b), dim3(1024), 0, current_stream(), n, cap, keep, xyz, out, counts);
  check_launch("compact_frames_scan");
}

extern "C" void sweep_filter_compact_kernel_wrapper(int S, int R, int cap, const int *lengths, const float *sweeps, int dataset,
                                                    const double *tr, float ground_z, float near, float *packed, int *counts) {
  if (S <= 0) return;
  PWCLO_REQUIRE(R > 0 && cap > 0 && (long long)R * 4 < (1ll << 31) && (long long)cap * 3 < (1ll << 31),
                "sweep_filter_compact: R=%d cap=%d out of range", R, cap);
  PWCLO_REQUIRE(dataset == 0 || dataset == 1, "sweep_filter_compact: dataset=%d (0 = KITTI, 1 = KITTI-360)", dataset);
  PWCLO_REQUIRE(lengths != nullptr && sweeps != nullptr && packed != nullptr && counts != nullptr &&
                (dataset == 1 || tr != nullptr), "sweep_filter_compact: lengths, sweeps, outputs (and tr for KITTI) are required%s", "");
  PWCLO_REQUIRE((reinterpret_cast<uintptr_t>(sweeps) & 15) == 0, "sweep_filter_compact: sweeps must be 16-byte aligned%s", "");
  if (dataset == 0)
    hipLaunchKernelGGL(sweep_filter_compact_kernel<true>, dim3(S), dim3(1024), 0, current_stream(), R, cap, lengths, sweeps,
                       tr, ground_z, near, packed, counts);
  else
    hipLaunchKernelGGL(sweep_filter_compact_kernel<false>, dim3(S), dim3(1024), 0, current_stream(), R, cap, lengths, sweeps,
                       tr, ground_z, near, packed, counts);
  check_launch("sweep_filter_compact");
}

extern "C" void ingest_frames_kernel_wrapper(int b, int n, int n_total, int c, const float *frame1,
                                             const float *frame2, float *out) {
  if (b <= 0 || n <= 0) return;
  PWCLO_REQUIRE(2 * b <= 65535, "ingest_frames: b=%d exceeds the grid limit", b);
  PWCLO_REQUIRE(c >= 3 && n_total >= n, "ingest_frames: need c >= 3 and n_total >= n (c=%d n_total=%d n=%d)", c,
                n_total, n);
  hipLaunchKernelGGL(ingest_frames_kernel, dim3(ceil_div(n, 256), 2 * b), dim3(256), 0, current_stream(), b, n,
                     n_total, c, frame1, frame2, out);
  check_launch("ingest_frames");
}

extern "C" void ingest_sequence_kernel_wrapper(int t, int n, int n_total, int c, const float *frames, float *out) {
  if (t <= 0 || n <= 0) return;
  PWCLO_REQUIRE(t <= 65535, "ingest_sequence: t=%d exceeds the grid limit", t);
  PWCLO_REQUIRE(c >= 3 && n_total >= n, "ingest_sequence: need c >= 3 and n_total >= n (c=%d n_total=%d n=%d)", c,
                n_total, n);
  hipLaunchKernelGGL(ingest_sequence_kernel, dim3(ceil_div(n, 256), t), dim3(256), 0, current_stream(), n, n_total, c,
                     frames, out);
  check_launch("ingest_sequence");
}

extern "C" void ingest_pairs_kernel_wrapper(int b, int n, const float *xyz_f1, const float *xyz_f2,
                                            float *out) {
  if (b <= 0 || n <= 0) return;
  PWCLO_REQUIRE(2 * b <= 65535, "ingest_pairs: b=%d exceeds the grid limit", b);
  hipLaunchKernelGGL(ingest_pairs_kernel, dim3(ceil_div(n, 256), 2 * b), dim3(256), 0, current_stream(), b, n,
                     xyz_f1, xyz_f2, out);
  check_launch("ingest_pairs");
}

// Hamilton product of two batches of quaternion rows, c[b][:, n] = a[b][:, n or 0] (x) b[b][:, n or 0], rows (B, 4, N)
// (PW/PWCLO_utils.py:83-95 mul_q_point and 117-129 mul_point_q: both are this product with the left operand's factors
// first).  Every product is rounded before the sums, left to right as the reference's torch expression, so the result
// is the expression's bit for bit.  conj_a / conj_b: use the conjugate (a0, -a1, -a2, -a3) of that operand -- the
// product's gradients are products with conjugates (dA = dC (x) conj(B), dB = conj(A) (x) dC), so the same kernel
// serves the backward.
namespace pwclo {
__global__ void hamilton_kernel(int n, int na, int nb, int conj_a, int conj_b, const float *__restrict__ a,
                                const float *__restrict__ b, float *__restrict__ c) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, bi = blockIdx.y;
  if (i >= n) return;
  const float *pa = a + (size_t)bi * 4 * na + (na == 1 ? 0 : i);
  const float *pb = b + (size_t)bi * 4 * nb + (nb == 1 ? 0 : i);
  const float sa = conj_a ? -1.f : 1.f, sb = conj_b ? -1.f : 1.f;
  const float a0 = pa[0], a1 = sa * pa[na], a2 = sa * pa[2 * na], a3 = sa * pa[3 * na];
  const float b0 = pb[0], b1 = sb * pb[nb], b2 = sb * pb[2 * nb], b3 = sb * pb[3 * nb];
  float *pc = c + (size_t)bi * 4 * n + i;
  auto m = [](float u, float v) { return __fmul_rn(u, v); };
  pc[0] = __fsub_rn(__fsub_rn(__fsub_rn(m(a0, b0), m(a1, b1)), m(a2, b2)), m(a3, b3));
  pc[n] = __fsub_rn(__fadd_rn(__fadd_rn(m(a0, b1), m(a1, b0)), m(a2, b3)), m(a3, b2));
  pc[2 * n] = __fadd_rn(__fadd_rn(__fsub_rn(m(a0, b2), m(a1, b3)), m(a2, b0)), m(a3, b1));
  pc[3 * n] = __fadd_rn(__fsub_rn(__fadd_rn(m(a0, b3), m(a1, b2)), m(a2, b1)), m(a3, b0));
}
}  // namespace pwclo

extern "C" void hamilton_product_kernel_wrapper(int b, int n, int na, int nb, int conj_a, int conj_b, const float *a,
                                                const float *q, float *out) {
  if (b <= 0 || n <= 0) return;
  PWCLO_REQUIRE(b <= 65535, "hamilton_product: b=%d exceeds the grid limit", b);
  PWCLO_REQUIRE((na == 1 || na == n) && (nb == 1 || nb == n), "hamilton_product: operand lengths %d, %d must be 1 or n=%d",
                na, nb, n);
  hipLaunchKernelGGL(pwclo::hamilton_kernel, dim3(ceil_div(n, 256), b), dim3(256), 0, current_stream(), n, na, nb, conj_a,
                     conj_b, a, q, out);
  check_launch("hamilton_product");
}

extern "C" void quat_warp_kernel_wrapper(int b, int n, const float *xyz, const float *q,
                                         const float *t, float *out) {
  if (b <= 0 || n <= 0) return;
  PWCLO_REQUIRE(b <= 65535, "quat_warp: b=%d exceeds the grid limit", b);
  hipLaunchKernelGGL(quat_warp_kernel<false>, dim3(ceil_div(n, 256), b), dim3(256), 0, current_stream(),
                     n, xyz, q, t, out);
  check_launch("quat_warp");
}

// Same transform on point-major (b,n,3) clouds (layout of the fused eval-mode pipeline).
extern "C" void quat_warp_pm_kernel_wrapper(int b, int n, const float *xyz, const float *q,
                                            const float *t, float *out) {
  if (b <= 0 || n <= 0) return;
  PWCLO_REQUIRE(b <= 65535, "quat_warp_pm: b=%d exceeds the grid limit", b);
  hipLaunchKernelGGL(quat_warp_kernel<true>, dim3(ceil_div(n, 256), b), dim3(256), 0, current_stream(),
                     n, xyz, q, t, out);
  check_launch("quat_warp_pm");
}
