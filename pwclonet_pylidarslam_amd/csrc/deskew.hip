// Motion compensation ("de-skewing") of raw sweeps with the last estimated motion (gfx950).
//
// A spinning LiDAR collects a sweep while the vehicle moves; the reference's `distortion` filter (slam/preprocessing.py:
// 131-191) moves row i by the fraction alpha_i of the constant-velocity prior (slam/initialization.py:106-122: the last
// registered relative pose): p'_i = slerp(I, R, alpha_i) p_i + alpha_i t, alpha_i the row's timestamp normalised to [0, 1]
// over the rows that survive the dataset filter.  deskew.hpp holds the row body; this file holds
//   deskew_rows_kernel                        the op alone (preprocess.deskew)
//   sweep_filter_deskew_compact_kernel        sweep_filter_compact_kernel (warp.hip) with the de-skew in it
//   sweep_filter_deskew_grid_compact_kernel   the same with section 19's grid between de-skew and compaction
//   stream_motion_handover_kernel             the motion a stream's next sweep gets, written after the append
// The keep decision is taken on the coordinates BEFORE de-skewing (the reference's dataset filters run before its
// Preprocessing block), so masks and survivor counts are those of the kernels without the step.  Every kernel is one
// 1024-thread workgroup per cloud, reads lengths, masks and the motion from device memory, allocates nothing and
// synchronises with nobody outside its workgroup: one captured graph serves every length and every motion.
#include <math.h>

#include "common.hpp"
#include "deskew.hpp"
#include "grid.hpp"
#include "rows.hpp"

namespace pwclo {

// points (b, n, stride) fp32, times (b, n) fp64, motion (b, 7) fp32 -> out (b, n, 3) fp32.  Candidates: rows below
// lengths[c] (nullable: all n) with keep_in != 0 (nullable: all).  Pass 1 reduces the candidates' finite times, pass 2
// transforms; every other row passes through with its bits.
__global__ __launch_bounds__(1024) void deskew_rows_kernel(int n, int stride, const float *__restrict__ points,
                                                           const double *__restrict__ times,
                                                           const float *__restrict__ motion,
                                                           const int *__restrict__ lengths,
                                                           const int *__restrict__ keep_in, float *__restrict__ out) {
  __shared__ double range_lds[32];
  const int c = blockIdx.x;
  const int len = lengths ? min(max(lengths[c], 0), n) : n;
  const float *pc = points + (size_t)c * n * stride;
  const double *tc = times + (size_t)c * n;
  const int *kin = keep_in ? keep_in + (size_t)c * n : nullptr;
  float *oc = out + (size_t)c * n * 3;
  const DeskewMotion m = deskew_motion(motion + (size_t)c * 7);
  DeskewRange mine = deskew_range_empty();
  for (int i = threadIdx.x; i < len; i += 1024)
    if (kin == nullptr || kin[i] != 0) deskew_range_add(mine, tc[i]);
  const DeskewRange range = deskew_range_reduce(mine, range_lds);
  for (int i = threadIdx.x; i < n; i += 1024) {
    const float p[3] = {pc[(size_t)i * stride], pc[(size_t)i * stride + 1], pc[(size_t)i * stride + 2]};
    const bool cand = i < len && (kin == nullptr || kin[i] != 0);
    float o[3];
    deskew_row(p, cand ? deskew_alpha(tc[i], range) : 0.0, m, o);
    oc[(size_t)i * 3 + 0] = o[0];
    oc[(size_t)i * 3 + 1] = o[1];
    oc[(size_t)i * 3 + 2] = o[2];
  }
}

// The motion of stream s in a fused front end: the identity when the stream primes in this call (per-stream mode: its
// restart word is set or it has no previous frame; both nullable, read from this call's device masks), else motion[s].
__device__ __forceinline__ DeskewMotion sweep_motion(int s, const float *__restrict__ motion,
                                                     const int *__restrict__ restart, const int *__restrict__ have_prev) {
  const bool primes = (restart != nullptr && restart[s] != 0) || (have_prev != nullptr && have_prev[s] == 0);
  return deskew_motion(primes ? nullptr : motion + (size_t)s * 7);
}

// sweep_filter_compact_kernel's layout (one workgroup per stream, wave w owns a contiguous range of rows, ballot / popcount
// counting pass, LDS scan of the 16 wave totals, writing pass that evaluates the row again).  The counting pass is already
// a full pass over the rows, so it also reduces the kept rows' time range; the writing pass evaluates filter + de-skew.
template <bool KITTI>
__global__ __launch_bounds__(1024) void sweep_filter_deskew_compact_kernel(
    int R, int cap, const int *__restrict__ lengths, const float *__restrict__ sweeps, const double *__restrict__ tr,
    float ground_z, float near, const double *__restrict__ times, const float *__restrict__ motion,
    const int *__restrict__ restart, const int *__restrict__ have_prev, float *__restrict__ packed,
    int *__restrict__ counts) {
  __shared__ int wave_total[16];
  __shared__ double range_lds[32];
  const int s = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = min(max(lengths[s], 0), R);
  const int per_wave = ((n + 15) / 16 + 63) / 64 * 64;          // multiple of 64: steps never straddle two waves' ranges
  const int i0 = wave * per_wave, i1 = min(n, i0 + per_wave);
  const float *sf = sweeps + (size_t)s * R * 4;
  const double *tc = times + (size_t)s * R;
  const double *ts = KITTI ? tr + (size_t)s * 12 : nullptr;
  const DeskewMotion m = sweep_motion(s, motion, restart, have_prev);
  auto row = [&](int i, float o[3]) {
    const float4 p = *reinterpret_cast<const float4 *>(sf + (size_t)i * 4);
    return KITTI ? kitti_row(p, ts, o) : kitti360_row(p, ground_z, near, o);
  };
  int total = 0;
  DeskewRange mine = deskew_range_empty();
  for (int i = i0 + lane; i - lane < i1; i += 64) {
    float o[3];
    const bool k = i < i1 && row(i, o);
    if (k) deskew_range_add(mine, tc[i]);
    total += __popcll(__ballot(k));
  }
  if (lane == 0) wave_total[wave] = total;
  const DeskewRange range = deskew_range_reduce(mine, range_lds);      // its barriers also publish wave_total
  int base = 0, all = 0;
  for (int w = 0; w < 16; ++w) {
    const int t = wave_total[w];
    if (w < wave) base += t;
    all += t;
  }
  float *of = packed + (size_t)s * cap * 3;
  for (int i = i0 + lane; i - lane < i1; i += 64) {
    float f[3];
    const bool k = i < i1 && row(i, f);
    const unsigned long long mask = __ballot(k);
    const int p = base + mbcnt64(mask);
    if (k && p < cap) {
      float o[3];
      deskew_row(f, deskew_alpha(tc[i], range), m, o);
      of[(size_t)p * 3 + 0] = o[0];
      of[(size_t)p * 3 + 1] = o[1];
      of[(size_t)p * 3 + 2] = o[2];
    }
    base += __popcll(mask);
  }
  const int count = all < cap ? all : cap;
  for (size_t j = (size_t)count * 3 + threadIdx.x; j < (size_t)cap * 3; j += 1024) of[j] = 0.0f;   // disjoint from the survivors
  if (threadIdx.x == 0) counts[s] = count;
}

// sweep_filter_grid_compact_kernel (grid_sample.hip) on the de-skewed coordinates: the grid sees what the network sees.
// The time range must be known before the first key is made, so one more pass over the rows (filter + range) precedes
// the insert pass; insert and writing pass evaluate filter + de-skew.
template <bool KITTI>
__global__ __launch_bounds__(1024) void sweep_filter_deskew_grid_compact_kernel(
    int R, int cap, const int *__restrict__ lengths, const float *__restrict__ sweeps, const double *__restrict__ tr,
    float ground_z, float near, const double *__restrict__ times, const float *__restrict__ motion,
    const int *__restrict__ restart, const int *__restrict__ have_prev, double voxel, char *__restrict__ ws,
    float *__restrict__ packed, int *__restrict__ counts, int *__restrict__ winners) {
  __shared__ int wave_total[16];
  __shared__ double range_lds[32];
  const int s = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = min(max(lengths[s], 0), R);
  const int per_wave = ((n + 15) / 16 + 63) / 64 * 64;
  const int i0 = wave * per_wave, i1 = min(n, i0 + per_wave);
  const float *sf = sweeps + (size_t)s * R * 4;
  const double *tc = times + (size_t)s * R;
  const double *ts = KITTI ? tr + (size_t)s * 12 : nullptr;
  const DeskewMotion m = sweep_motion(s, motion, restart, have_prev);
  auto row = [&](int i, float o[3]) {
    const float4 p = *reinterpret_cast<const float4 *>(sf + (size_t)i * 4);
    return KITTI ? kitti_row(p, ts, o) : kitti360_row(p, ground_z, near, o);
  };
  const GridTable t = grid_table(ws, s, R, n);
  int *mark = reinterpret_cast<int *>(ws + (long long)s * grid_layout(R).stride + grid_layout(R).slots_off);
  grid_clear(t);
  DeskewRange mine = deskew_range_empty();
  for (int i = i0 + lane; i < i1; i += 64) {
    float o[3];
    if (row(i, o)) deskew_range_add(mine, tc[i]);
  }
  const DeskewRange range = deskew_range_reduce(mine, range_lds);
  auto moved = [&](int i, float o[3]) {                  // filter, then the kept row de-skewed
    float f[3];
    const bool k = row(i, f);
    deskew_row(f, k ? deskew_alpha(tc[i], range) : 0.0, m, o);
    return k;
  };
  grid_phase_barrier();
  for (int i = i0 + lane; i < i1; i += 64) {
    float o[3];
    unsigned long long h;
    const bool cand = moved(i, o) && grid_key(o, voxel, h);
    mark[i] = cand ? grid_insert(t, h, (unsigned)i) : -1;
  }
  grid_phase_barrier();
  int total = 0;
  for (int i = i0 + lane; i - lane < i1; i += 64) {
    bool w = false;
    if (i < i1) {
      const int slot = mark[i];
      w = slot >= 0 && grid_is_winner(t, slot, (unsigned)i);
      mark[i] = w ? 1 : 0;
    }
    total += __popcll(__ballot(w));
  }
  if (lane == 0) wave_total[wave] = total;
  __syncthreads();
  int base = 0, all = 0;
  for (int w = 0; w < 16; ++w) {
    const int tw = wave_total[w];
    if (w < wave) base += tw;
    all += tw;
  }
  float *of = packed + (size_t)s * cap * 3;
  for (int i = i0 + lane; i - lane < i1; i += 64) {
    const bool k = i < i1 && mark[i] != 0;
    const unsigned long long mask = __ballot(k);
    const int p = base + mbcnt64(mask);
    if (k && p < cap) {
      float o[3];
      moved(i, o);
      of[(size_t)p * 3 + 0] = o[0];
      of[(size_t)p * 3 + 1] = o[1];
      of[(size_t)p * 3 + 2] = o[2];
    }
    base += __popcll(mask);
  }
  const int count = all < cap ? all : cap;
  for (size_t j = (size_t)count * 3 + threadIdx.x; j < (size_t)cap * 3; j += 1024) of[j] = 0.0f;   // disjoint from the survivors
  if (threadIdx.x == 0) {
    counts[s] = count;
    winners[s] = all;
  }
}

// After the append: the motion the next sweep of stream s is de-skewed with (ConstantVelocityInitialization: the relative
// pose registered last).  One thread per stream.  active (nullable: every stream): an idle stream's motion stays as it is.
// rows (nullable: the identity for every active stream): stream s's level-1 pose row at rows + s * row_stride; the masked append has
// already turned the rows of streams that primed into the identity, so a primed stream hands over the identity too.
__global__ __launch_bounds__(1024) void stream_motion_handover_kernel(int S, const int *__restrict__ active,
                                                                      const float *__restrict__ rows, int row_stride,
                                                                      float *__restrict__ motion) {
  const int i = threadIdx.x;
  if (i >= S) return;
  if (active != nullptr && active[i] == 0) return;
#pragma unroll
  for (int j = 0; j < 7; ++j)
    motion[(size_t)i * 7 + j] = rows != nullptr ? rows[(size_t)i * row_stride + j] : (j == 3 ? 1.0f : 0.0f);
}

}  // namespace pwclo

using namespace pwclo;

extern "C" void deskew_rows_kernel_wrapper(int b, int n, int stride, const float *points, const double *times,
                                           const float *motion, const int *lengths, const int *keep_in, float *xyz) {
  if (b <= 0 || n <= 0) return;
  PWCLO_REQUIRE(b <= 65535 && (long long)n * 4 < (1ll << 31), "deskew_rows: b=%d n=%d out of range", b, n);
  PWCLO_REQUIRE(stride == 3 || stride == 4, "deskew_rows: row stride %d (3 or 4 floats)", stride);
  PWCLO_REQUIRE(points != nullptr && times != nullptr && motion != nullptr && xyz != nullptr,
                "deskew_rows: points, times, motion and the output are required%s", "");
  PWCLO_REQUIRE((reinterpret_cast<uintptr_t>(times) & 7) == 0, "deskew_rows: times must be 8-byte aligned%s", "");
  hipLaunchKernelGGL(deskew_rows_kernel, dim3(b), dim3(1024), 0, current_stream(), n, stride, points, times, motion, lengths,
                     keep_in, xyz);
  check_launch("deskew_rows");
}

extern "C" void sweep_filter_deskew_compact_kernel_wrapper(int S, int R, int cap, const int *lengths, const float *sweeps,
                                                           int dataset, const double *tr, float ground_z, float near,
                                                           const double *times, const float *motion, const int *restart,
                                                           const int *have_prev, float *packed, int *counts) {
  if (S <= 0) return;
  PWCLO_REQUIRE(R > 0 && cap > 0 && (long long)R * 4 < (1ll << 31) && (long long)cap * 3 < (1ll << 31),
                "sweep_filter_deskew_compact: R=%d cap=%d out of range", R, cap);
  PWCLO_REQUIRE(dataset == 0 || dataset == 1, "sweep_filter_deskew_compact: dataset=%d (0 = KITTI, 1 = KITTI-360)", dataset);
  PWCLO_REQUIRE(lengths != nullptr && sweeps != nullptr && times != nullptr && motion != nullptr && packed != nullptr &&
                counts != nullptr && (dataset == 1 || tr != nullptr),
                "sweep_filter_deskew_compact: lengths, sweeps, times, motion, outputs (and tr for KITTI) are required%s", "");
  PWCLO_REQUIRE((reinterpret_cast<uintptr_t>(sweeps) & 15) == 0 && (reinterpret_cast<uintptr_t>(times) & 7) == 0,
                "sweep_filter_deskew_compact: sweeps must be 16-byte and times 8-byte aligned%s", "");
  if (dataset == 0)
    hipLaunchKernelGGL(sweep_filter_deskew_compact_kernel<true>, dim3(S), dim3(1024), 0, current_stream(), R, cap, lengths,
                       sweeps, tr, ground_z, near, times, motion, restart, have_prev, packed, counts);
  else
    hipLaunchKernelGGL(sweep_filter_deskew_compact_kernel<false>, dim3(S), dim3(1024), 0, current_stream(), R, cap, lengths,
                       sweeps, tr, ground_z, near, times, motion, restart, have_prev, packed, counts);
  check_launch("sweep_filter_deskew_compact");
}

extern "C" void sweep_filter_deskew_grid_compact_kernel_wrapper(int S, int R, int cap, const int *lengths, const float *sweeps,
                                                                int dataset, const double *tr, float ground_z, float near,
                                                                const double *times, const float *motion,
                                                                const int *restart, const int *have_prev, double voxel,
                                                                void *workspace, float *packed, int *counts, int *winners) {
  if (S <= 0) return;
  PWCLO_REQUIRE(R > 0 && R <= GRID_MAX_ROWS && cap > 0 && (long long)cap * 3 < (1ll << 31),
                "sweep_filter_deskew_grid_compact: R=%d cap=%d out of range (R <= %d)", R, cap, GRID_MAX_ROWS);
  PWCLO_REQUIRE(dataset == 0 || dataset == 1, "sweep_filter_deskew_grid_compact: dataset=%d (0 = KITTI, 1 = KITTI-360)",
                dataset);
  PWCLO_REQUIRE(grid_voxel_ok(voxel), "sweep_filter_deskew_grid_compact: voxel=%g must be finite and > 0", voxel);
  PWCLO_REQUIRE(lengths != nullptr && sweeps != nullptr && times != nullptr && motion != nullptr && workspace != nullptr &&
                packed != nullptr && counts != nullptr && winners != nullptr && (dataset == 1 || tr != nullptr),
                "sweep_filter_deskew_grid_compact: lengths, sweeps, times, motion, workspace, outputs (and tr for KITTI) are "
                "required%s", "");
  PWCLO_REQUIRE((reinterpret_cast<uintptr_t>(sweeps) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0 &&
                (reinterpret_cast<uintptr_t>(times) & 7) == 0,
                "sweep_filter_deskew_grid_compact: sweeps must be 16-byte, workspace and times 8-byte aligned%s", "");
  char *ws = static_cast<char *>(workspace);
  if (dataset == 0)
    hipLaunchKernelGGL(sweep_filter_deskew_grid_compact_kernel<true>, dim3(S), dim3(1024), 0, current_stream(), R, cap,
                       lengths, sweeps, tr, ground_z, near, times, motion, restart, have_prev, voxel, ws, packed, counts,
                       winners);
  else
    hipLaunchKernelGGL(sweep_filter_deskew_grid_compact_kernel<false>, dim3(S), dim3(1024), 0, current_stream(), R, cap,
                       lengths, sweeps, tr, ground_z, near, times, motion, restart, have_prev, voxel, ws, packed, counts,
                       winners);
  check_launch("sweep_filter_deskew_grid_compact");
}

extern "C" void stream_motion_handover_kernel_wrapper(int S, const int *active, const float *rows, int row_stride,
                                                      float *motion) {
  PWCLO_REQUIRE(S >= 1 && S <= 1024, "stream_motion_handover: S=%d streams outside one workgroup [1, 1024]", S);
  PWCLO_REQUIRE(motion != nullptr && (rows == nullptr || row_stride >= 7),
                "stream_motion_handover: motion is required and a row holds 7 floats (stride %d)", row_stride);
  hipLaunchKernelGGL(stream_motion_handover_kernel, dim3(1), dim3(ceil_div(S, 64) * 64), 0, current_stream(), S, active, rows,
                     row_stride, motion);
  check_launch("stream_motion_handover");
}
