// Voxel grid sampling of raw sweeps (gfx950): keep one row per occupied voxel, the lowest-index one.
//
// The rule (the reference's `grid_sample` filter, slam/common/pointcloud.py:105-130, with a stable output order):
//   q_a = rint(double(p_a) / v)   true fp64 division, round half to even
//   h   = 73856093 q_x + 19349669 q_y + 83492791 q_z   in 64 bits with wraparound
//   row i is a winner iff no lower-index candidate row of its cloud has the same h
// A row with a non-finite coordinate or |p_a / v| >= 2^31 on an axis is no candidate.
//
// One 1024-thread workgroup per cloud deduplicates through an open-addressing table in a caller-provided workspace:
//   clear   the cloud's T = 2^L >= 2 * length key slots (all ones = empty) and row words (all ones = no row yet)
//   insert  every candidate claims the first slot of its probe sequence that is empty or already holds its key (64-bit
//           compare-and-swap), then lowers that slot's row word to its own index (32-bit atomic min).  The minimum does
//           not depend on the order in which rows arrive, so the result is deterministic.
//   resolve a candidate is a winner iff its slot's row word is its own index
// The key whose bit pattern is the empty marker never enters the table: it owns one extra row word behind the T slots.
// Every table access is an agent-scope atomic (the loads too: the atomics execute in L2 and never refresh this CU's L1),
// and a `s_waitcnt vmcnt(0)` + workgroup barrier separates the phases.  Nothing outlives the launch: the table is cleared
// by the launch that uses it, so a replay on persistent buffers never sees an earlier sweep's keys.
#include <math.h>

#include "common.hpp"
#include "grid.hpp"
#include "rows.hpp"

namespace pwclo {

// The stand-alone op: points (b, n, stride) fp32 -> keep_out (b, n) i32 (1 for the winners), counts (b) i32.  Rows at or
// past lengths[c] (nullable: all n rows) and rows with keep_in == 0 (nullable) are no candidates.  Thread t owns rows
// t, t + 1024, ... in both passes and parks each candidate's slot in keep_out between them.
__global__ __launch_bounds__(1024) void grid_sample_keep_kernel(int n, int stride, const float *__restrict__ points,
                                                                const int *__restrict__ lengths,
                                                                const int *__restrict__ keep_in, double voxel,
                                                                char *__restrict__ ws, int *__restrict__ keep_out,
                                                                int *__restrict__ counts) {
  __shared__ int wave_total[16];
  const int c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int len = lengths ? min(max(lengths[c], 0), n) : n;
  const GridTable t = grid_table(ws, c, n, len);
  const float *pc = points + (size_t)c * n * stride;
  const int *kin = keep_in ? keep_in + (size_t)c * n : nullptr;
  int *kout = keep_out + (size_t)c * n;
  grid_clear(t);
  grid_phase_barrier();
  for (int i = threadIdx.x; i < len; i += 1024) {
    const float o[3] = {pc[(size_t)i * stride], pc[(size_t)i * stride + 1], pc[(size_t)i * stride + 2]};
    unsigned long long h;
    const bool cand = grid_key(o, voxel, h) && (kin == nullptr || kin[i] != 0);
    kout[i] = cand ? grid_insert(t, h, (unsigned)i) : -1;
  }
  grid_phase_barrier();
  int total = 0;
  for (int i = threadIdx.x; i - (int)threadIdx.x < n; i += 1024) {      // whole waves: the ballot counts the winners
    bool w = false;
    if (i < len) {
      const int slot = kout[i];
      w = slot >= 0 && grid_is_winner(t, slot, (unsigned)i);
    }
    if (i < n) kout[i] = w ? 1 : 0;
    total += __popcll(__ballot(w));
  }
  if (lane == 0) wave_total[wave] = total;
  __syncthreads();
  if (threadIdx.x == 0) {
    int all = 0;
    for (int w = 0; w < 16; ++w) all += wave_total[w];
    counts[c] = all;
  }
}

// sweep_filter_compact_kernel (warp.hip) with the grid between the filter and the compaction: same layout (one 1024-thread
// workgroup per stream, wave w owns a contiguous range of rows, ballot / popcount counting pass, LDS scan of the 16 wave
// totals, writing pass that evaluates the row again), same row bodies, so the survivors' coordinate bits are the same.
// A row is a candidate iff the filter keeps it.  The insert pass parks each row's slot in the workspace, the counting pass
// replaces it by the winner flag, the writing pass reads the flag: a thread only ever reads back what it wrote itself.
// winners[s] = the number of winners, counts[s] = min(winners, cap); rows [counts, cap) of packed are zeroed.
template <bool KITTI>
__global__ __launch_bounds__(1024) void sweep_filter_grid_compact_kernel(int R, int cap, const int *__restrict__ lengths,
                                                                         const float *__restrict__ sweeps,
                                                                         const double *__restrict__ tr, float ground_z,
                                                                         float near, double voxel, char *__restrict__ ws,
                                                                         float *__restrict__ packed,
                                                                         int *__restrict__ counts,
                                                                         int *__restrict__ winners) {
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
  const GridTable t = grid_table(ws, s, R, n);
  int *mark = reinterpret_cast<int *>(ws + (long long)s * grid_layout(R).stride + grid_layout(R).slots_off);
  grid_clear(t);
  grid_phase_barrier();
  for (int i = i0 + lane; i < i1; i += 64) {
    float o[3];
    unsigned long long h;
    const bool cand = row(i, o) && grid_key(o, voxel, h);
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
    const unsigned long long m = __ballot(k);
    const int p = base + mbcnt64(m);
    if (k && p < cap) {
      float o[3];
      row(i, o);
      of[(size_t)p * 3 + 0] = o[0];
      of[(size_t)p * 3 + 1] = o[1];
      of[(size_t)p * 3 + 2] = o[2];
    }
    base += __popcll(m);
  }
  const int count = all < cap ? all : cap;
  for (size_t j = (size_t)count * 3 + threadIdx.x; j < (size_t)cap * 3; j += 1024) of[j] = 0.0f;   // disjoint from the survivors
  if (threadIdx.x == 0) {
    counts[s] = count;
    winners[s] = all;
  }
}

}  // namespace pwclo

using namespace pwclo;

extern "C" long long grid_sample_workspace_bytes(int b, int n) {
  if (b <= 0 || n <= 0 || n > GRID_MAX_ROWS) return 0;
  return (long long)b * grid_layout(n).stride;
}

extern "C" void grid_sample_keep_kernel_wrapper(int b, int n, int stride, const float *points, const int *lengths,
                                                const int *keep_in, double voxel, void *workspace, int *keep_out,
                                                int *counts) {
  if (b <= 0 || n <= 0) return;
  PWCLO_REQUIRE(n <= GRID_MAX_ROWS, "grid_sample_keep: n=%d rows per cloud above %d", n, GRID_MAX_ROWS);
  PWCLO_REQUIRE(stride == 3 || stride == 4, "grid_sample_keep: row stride %d (3 or 4 floats)", stride);
  PWCLO_REQUIRE(grid_voxel_ok(voxel), "grid_sample_keep: voxel=%g must be finite and > 0", voxel);
  PWCLO_REQUIRE(points != nullptr && workspace != nullptr && keep_out != nullptr && counts != nullptr,
                "grid_sample_keep: points, workspace and outputs are required%s", "");
  PWCLO_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "grid_sample_keep: workspace must be 8-byte aligned%s", "");
  hipLaunchKernelGGL(grid_sample_keep_kernel, dim3(b), dim3(1024), 0, current_stream(), n, stride, points, lengths, keep_in,
                     voxel, static_cast<char *>(workspace), keep_out, counts);
  check_launch("grid_sample_keep");
}

extern "C" void sweep_filter_grid_compact_kernel_wrapper(int S, int R, int cap, const int *lengths, const float *sweeps,
                                                         int dataset, const double *tr, float ground_z, float near,
                                                         double voxel, void *workspace, float *packed, int *counts,
                                                         int *winners) {
  if (S <= 0) return;
  PWCLO_REQUIRE(R > 0 && R <= GRID_MAX_ROWS && cap > 0 && (long long)cap * 3 < (1ll << 31),
                "sweep_filter_grid_compact: R=%d cap=%d out of range (R <= %d)", R, cap, GRID_MAX_ROWS);
  PWCLO_REQUIRE(dataset == 0 || dataset == 1, "sweep_filter_grid_compact: dataset=%d (0 = KITTI, 1 = KITTI-360)", dataset);
  PWCLO_REQUIRE(grid_voxel_ok(voxel), "sweep_filter_grid_compact: voxel=%g must be finite and > 0", voxel);
  PWCLO_REQUIRE(lengths != nullptr && sweeps != nullptr && workspace != nullptr && packed != nullptr && counts != nullptr &&
                winners != nullptr && (dataset == 1 || tr != nullptr),
                "sweep_filter_grid_compact: lengths, sweeps, workspace, outputs (and tr for KITTI) are required%s", "");
  PWCLO_REQUIRE((reinterpret_cast<uintptr_t>(sweeps) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
                "sweep_filter_grid_compact: sweeps must be 16-byte and the workspace 8-byte aligned%s", "");
  char *ws = static_cast<char *>(workspace);
  if (dataset == 0)
    hipLaunchKernelGGL(sweep_filter_grid_compact_kernel<true>, dim3(S), dim3(1024), 0, current_stream(), R, cap, lengths,
                       sweeps, tr, ground_z, near, voxel, ws, packed, counts, winners);
  else
    hipLaunchKernelGGL(sweep_filter_grid_compact_kernel<false>, dim3(S), dim3(1024), 0, current_stream(), R, cap, lengths,
                       sweeps, tr, ground_z, near, voxel, ws, packed, counts, winners);
  check_launch("sweep_filter_grid_compact");
}
