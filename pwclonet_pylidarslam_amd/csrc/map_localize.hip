// Localisation of a frame in the global map (gfx950): point-to-plane registration of a cloud against
// the voxel-hashed world map of global_map.hip, with the plane of every pair fitted from the map's own neighbourhood.
//
// The map's table (grid.hpp) sends a key to a slot and the slot's row word to a global row id; the world point of that row
// lives at its rank in `points`.  The localiser therefore owns index (S, T + 1) ints, slot -> rank (slot T: the empty
// marker's voxel), filled by map_index_kernel from the ranks themselves.  An entry is never trusted: slot s found for the
// key h yields the candidate r = index[s] only where 0 <= r < M = min(total, capacity), grid_key(points[r]) is valid and
// equals h, and (max_source_frame given) source[r][0] <= max_source_frame[s].  The map holds one point per key, so a
// lookup returns the map's point of that voxel or nothing; a stale entry can hide a point, never return a wrong one.
//
//   map_index_kernel                 ranks [lo, M): the key of points[r], a read-only probe, index[slot] = r (lo = 0 for a
//                                    full pass and for the streams of the refill word: their map was emptied since)
//   map_index_end_kernel             indexed[s] = M
//   map_localize_begin_kernel        T <- init for the active streams
//   map_localize_accumulate_kernel   q = fp32(T p); the (2R + 1)^3 voxels around q in dz, dy, dx order; the nearest candidate;
//                                    mean, covariance, icp_eig3 and the rank test over all candidates; the row of sums
// The solver is icp_solve_kernel, unchanged.  Nothing here writes a buffer of the map, no access is atomic (a kernel
// boundary separates every writer from its readers), no loop waits on another workgroup and every fp64 sum is added in
// the candidate order by one thread, then by icp_reduce_store_row: two runs give the same bits.
//
// Form of the accumulate kernel: one thread per query, templated on R.  The voxels are handled in batches of B (27 for R =
// 1: one batch; 25 for R = 2: the five dz planes), and inside a batch each stage runs over all B voxels before the next
// begins: all keys and home slots, all key loads, the (rare) further probes, all index loads, all point loads, then the
// validation and the sums in order.  The loads of a stage do not depend on each other, so they are in flight together
// instead of one round trip per voxel.
#include <math.h>

#include "common.hpp"
#include "grid.hpp"
#include "icp.hpp"
#include "se3.hpp"

namespace pwclo {

constexpr int ML_MAX_STREAMS = 1024;
constexpr int ML_BLOCK = 256;

struct MlMap {
  int log2T, capacity;
  double voxel;
  const unsigned long long *keys;      // (S, T)
  const float *points;                 // (S, capacity, 3)
  const int *source;                   // (S, capacity, 2)
  const int *total;                    // word s at total[s * total_stride]
  int total_stride;
  __device__ __forceinline__ int T() const { return 1 << log2T; }
  __device__ __forceinline__ int ranks(int s) const { return min(max(total[(size_t)s * total_stride], 0), capacity); }
};

// grid_key's hash from integer voxel coordinates.
__device__ __forceinline__ unsigned long long ml_voxel_key(long long cx, long long cy, long long cz) {
  return 73856093ull * (unsigned long long)cx + 19349669ull * (unsigned long long)cy + 83492791ull * (unsigned long long)cz;
}

__device__ __forceinline__ int ml_home(unsigned long long h, int log2T) {
  return h == GRID_EMPTY ? (1 << log2T) : (int)((h * 0x9E3779B97F4A7C15ull) >> (64 - log2T));
}

// From `slot` (a home slot < T whose key `cur` has been read): the slot that holds h, -1 where an empty slot comes first.
__device__ __forceinline__ int ml_probe(const unsigned long long *__restrict__ keys, int T, unsigned long long h, int slot,
                                        unsigned long long cur) {
  for (int step = 0; step < T; ++step) {
    if (cur == h) return slot;
    if (cur == GRID_EMPTY) return -1;
    slot = (slot + 1) & (T - 1);
    cur = keys[slot];
  }
  return -1;
}

// Grid (ceil(capacity / 256), S).  full != 0, or refill[s] != 0 (refill nullable): ranks [0, M); else [indexed[s], M).
__global__ __launch_bounds__(ML_BLOCK) void map_index_kernel(MlMap m, int full, const int *__restrict__ refill,
                                                             const int *__restrict__ indexed, int *__restrict__ index) {
  const int s = blockIdx.y;
  const int M = m.ranks(s), lo = (full || (refill != nullptr && refill[s] != 0)) ? 0 : max(indexed[s], 0);
  const long long r = (long long)lo + (long long)blockIdx.x * ML_BLOCK + threadIdx.x;
  if (r >= M) return;
  const int T = m.T();
  const float *pr = m.points + ((size_t)s * m.capacity + (size_t)r) * 3;
  const float pt[3] = {pr[0], pr[1], pr[2]};
  unsigned long long h;
  if (!grid_key(pt, m.voxel, h)) return;
  const unsigned long long *keys = m.keys + (size_t)s * T;
  int slot = ml_home(h, m.log2T);
  if (slot < T) slot = ml_probe(keys, T, h, slot, keys[slot]);
  if (slot >= 0) index[(size_t)s * (T + 1) + slot] = (int)r;
}

__global__ void map_index_end_kernel(int S, MlMap m, int *__restrict__ indexed) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < S) indexed[s] = m.ranks(s);
}

__global__ void map_localize_begin_kernel(int S, const double *__restrict__ init, const int *__restrict__ active,
                                          double *__restrict__ T) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S || (active != nullptr && active[s] == 0)) return;
#pragma unroll
  for (int e = 0; e < 16; ++e) T[(size_t)s * 16 + e] = init[(size_t)s * 16 + e];
}

// p (S, n, 3); T (S, 4, 4) or nullptr (q = p, the sensor at the origin) -> partial (S, gridDim.x, ICP_ROW).  rank / count /
// dist (S, n) and normal (S, n, 3), or all nullptr: the nearest candidate, the number of candidates and the plane of
// every point (-1, count, +Inf, 0 where there is none).
template <int R>
__global__ __launch_bounds__(ICP_ACC_THREADS) void map_localize_accumulate_kernel(
    MlMap m, int n, const float *__restrict__ p, const double *__restrict__ T, const int *__restrict__ index,
    const int *__restrict__ max_source_frame, double sigma, float max_dist, int min_neighbours,
    double *__restrict__ partial, int *__restrict__ rank_out, int *__restrict__ count_out, float *__restrict__ dist_out,
    float *__restrict__ normal_out, const int *__restrict__ active) {
  constexpr int W = 2 * R + 1, N = W * W * W, B = R == 1 ? 27 : 25, NB = N / B, U = R == 1 ? N : 5;
  static_assert(NB * B == N, "batches cover the block");
  const int s = blockIdx.y, i = blockIdx.x * ICP_ACC_THREADS + threadIdx.x;
  if (active != nullptr && active[s] == 0) {              // idle: a zero row, nothing read (the whole workgroup leaves)
    icp_store_zero_row(partial, s);
    return;
  }
  double acc[ICP_TERMS];
#pragma unroll
  for (int e = 0; e < ICP_TERMS; ++e) acc[e] = 0.0;
  if (i < n) {
    const Se3 t = T != nullptr ? se3_load(T + (size_t)s * 16) : se3_identity();
    const float *pr = p + ((size_t)s * n + i) * 3;
    const float pp[3] = {pr[0], pr[1], pr[2]};
    float q[3] = {pp[0], pp[1], pp[2]};
    if (T != nullptr) {
      double o[3];
      se3_apply(t, pp, o);
      q[0] = (float)o[0]; q[1] = (float)o[1]; q[2] = (float)o[2];
    }
    bool usable = true;
    long long c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double d = (double)q[a] / m.voxel;
      const bool in = fabs(d) < 2147483648.0;              // false for NaN and for +-inf
      usable = usable && in;
      c[a] = (long long)rint(in ? d : 0.0);
    }
    const int Tn = m.T(), M = m.ranks(s);
    const unsigned long long *keys = m.keys + (size_t)s * Tn;
    const int *idx = index + (size_t)s * (Tn + 1);
    const float *pts = m.points + (size_t)s * m.capacity * 3;
    const int *src = m.source + (size_t)s * m.capacity * 2;
    const bool gated = max_source_frame != nullptr;
    const int newest = gated ? max_source_frame[s] : 0;
    int rk[N];
    int best = -1, count = 0;
    float bd = INFINITY;
    double sum[3] = {0.0, 0.0, 0.0};
    if (usable) {
#pragma unroll 1
      for (int b = 0; b < NB; ++b) {
        unsigned long long h[B], cur[B];
        int slot[B], r[B];
        float pt[B][3];
#pragma unroll
        for (int j = 0; j < B; ++j) {                      // keys and home slots
          const int jj = b * B + j;
          const long long cx = c[0] + (jj % W - R), cy = c[1] + ((jj / W) % W - R), cz = c[2] + (jj / (W * W) - R);
          const bool in = llabs(cx) < 2147483648ll && llabs(cy) < 2147483648ll && llabs(cz) < 2147483648ll;
          h[j] = ml_voxel_key(cx, cy, cz);
          slot[j] = in ? ml_home(h[j], m.log2T) : -1;
        }
#pragma unroll
        for (int j = 0; j < B; ++j) cur[j] = (slot[j] >= 0 && slot[j] < Tn) ? keys[slot[j]] : GRID_EMPTY;
#pragma unroll
        for (int j = 0; j < B; ++j)
          if (slot[j] >= 0 && slot[j] < Tn) slot[j] = ml_probe(keys, Tn, h[j], slot[j], cur[j]);
#pragma unroll
        for (int j = 0; j < B; ++j) r[j] = slot[j] >= 0 ? idx[slot[j]] : -1;
#pragma unroll
        for (int j = 0; j < B; ++j) {
          if (r[j] < 0 || r[j] >= M) r[j] = -1;
          if (r[j] >= 0 && gated && src[(size_t)r[j] * 2] > newest) r[j] = -1;
        }
#pragma unroll
        for (int j = 0; j < B; ++j) {
          const size_t at = (size_t)(r[j] >= 0 ? r[j] : 0) * 3;
          pt[j][0] = r[j] >= 0 ? pts[at] : 0.0f;
          pt[j][1] = r[j] >= 0 ? pts[at + 1] : 0.0f;
          pt[j][2] = r[j] >= 0 ? pts[at + 2] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < B; ++j) {                      // validation, then the sums in candidate order
          unsigned long long hk;
          const bool ok = r[j] >= 0 && grid_key(pt[j], m.voxel, hk) && hk == h[j];
          rk[b * B + j] = ok ? r[j] : -1;
          if (!ok) continue;
          ++count;
          sum[0] += (double)pt[j][0]; sum[1] += (double)pt[j][1]; sum[2] += (double)pt[j][2];
          const float ex = q[0] - pt[j][0], ey = q[1] - pt[j][1], ez = q[2] - pt[j][2];
          const float d = sqrtf((ex * ex + ey * ey) + ez * ez);
          if (best < 0 || d < bd) {                        // strict: the first candidate stays on a tie
            best = r[j];
            bd = d;
          }
        }
      }
    }
    float nn[3] = {0.0f, 0.0f, 0.0f};
    if (best >= 0 && count >= min_neighbours && bd <= max_dist) {
      const double mu[3] = {sum[0] / (double)count, sum[1] / (double)count, sum[2] / (double)count};
      double cov[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll U
      for (int j = 0; j < N; ++j) {
        const int r = rk[j];
        if (r < 0) continue;
        const double d0 = (double)pts[(size_t)r * 3] - mu[0], d1 = (double)pts[(size_t)r * 3 + 1] - mu[1],
                     d2 = (double)pts[(size_t)r * 3 + 2] - mu[2];
        cov[0] += d0 * d0; cov[1] += d0 * d1; cov[2] += d0 * d2;
        cov[3] += d1 * d1; cov[4] += d1 * d2; cov[5] += d2 * d2;
      }
      double val[3], vec[3];
      icp_eig3(cov, val, vec);
      const float y[3] = {pts[(size_t)best * 3], pts[(size_t)best * 3 + 1], pts[(size_t)best * 3 + 2]};
      if (val[1] > ICP_RANK_EPS * val[2]) {
        const double d = (vec[0] * ((double)y[0] - t.m[3]) + vec[1] * ((double)y[1] - t.m[7])) +
                         vec[2] * ((double)y[2] - t.m[11]);
        const double sg = d > 0.0 ? -1.0 : 1.0;            // towards the sensor: n . (y - t) <= 0
        nn[0] = (float)(sg * vec[0]); nn[1] = (float)(sg * vec[1]); nn[2] = (float)(sg * vec[2]);
      }
      if (nn[0] != 0.0f || nn[1] != 0.0f || nn[2] != 0.0f) {
        const double eye[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
        icp_add_pair(pp, q, y, nn, t, eye, sigma, acc);
      }
    }
    if (rank_out != nullptr) {
      const size_t at = (size_t)s * n + i;
      rank_out[at] = best;
      count_out[at] = count;
      dist_out[at] = bd;
      normal_out[at * 3] = nn[0]; normal_out[at * 3 + 1] = nn[1]; normal_out[at * 3 + 2] = nn[2];
    }
  }
  icp_reduce_store_row(acc, partial, s);
}

}  // namespace pwclo

using namespace pwclo;

static int ml_log2T(long long T) {
  for (int L = 6; L <= 30; ++L)
    if ((1ll << L) == T) return L;
  return -1;
}

extern "C" long long map_localize_index_bytes(int S, long long T) {
  if (S < 1 || S > ML_MAX_STREAMS || ml_log2T(T) < 0) return 0;
  return (long long)S * 4 * (T + 1);
}

#define ML_MAP_ARGS(what)                                                                                                  \
  PWCLO_REQUIRE(S >= 1 && S <= ML_MAX_STREAMS, what ": S=%d outside [1, %d]", S, ML_MAX_STREAMS);                            \
  PWCLO_REQUIRE(ml_log2T(T) >= 0, what ": T=%lld must be a power of two in [2^6, 2^30]", T);                                 \
  PWCLO_REQUIRE(capacity >= 1 && (long long)capacity <= (1ll << 29), what ": capacity=%d outside [1, 2^29]", capacity);      \
  PWCLO_REQUIRE(grid_voxel_ok(voxel), what ": voxel=%g must be finite and > 0", voxel);                                      \
  PWCLO_REQUIRE(keys != nullptr && points != nullptr && source != nullptr && total != nullptr && index != nullptr &&         \
                total_stride >= 1, what ": keys, points, source, total (stride=%d >= 1) and index are required",            \
                total_stride);                                                                                             \
  PWCLO_REQUIRE(aligned(keys, 8) && aligned(points, 4) && aligned(source, 4) && aligned(total, 4) && aligned(index, 4),      \
                what ": keys must be 8-byte, the other arrays 4-byte aligned%s", "");                                       \
  const MlMap m = {ml_log2T(T), capacity, voxel, static_cast<const unsigned long long *>(keys), points, source, total,       \
                   total_stride}

extern "C" void map_index_kernel_wrapper(int S, long long T, int capacity, double voxel, const void *keys,
                                         const float *points, const int *source, const int *total, int total_stride,
                                         int full, const int *refill, int *indexed, int *index) {
  ML_MAP_ARGS("map_index");
  PWCLO_REQUIRE(indexed != nullptr && aligned(indexed, 4) && aligned(refill, 4), "map_index: indexed is required%s", "");
  hipLaunchKernelGGL(map_index_kernel, dim3(ceil_div(capacity, ML_BLOCK), S), dim3(ML_BLOCK), 0, current_stream(), m,
                     full != 0 ? 1 : 0, refill, indexed, index);
  hipLaunchKernelGGL(map_index_end_kernel, dim3(ceil_div(S, 64)), dim3(64), 0, current_stream(), S, m, indexed);
  check_launch("map_index");
}

extern "C" void map_localize_begin_kernel_wrapper(int S, const double *init, const int *active, double *Tm) {
  PWCLO_REQUIRE(S >= 1 && S <= ML_MAX_STREAMS, "map_localize_begin: S=%d outside [1, %d]", S, ML_MAX_STREAMS);
  PWCLO_REQUIRE(init != nullptr && Tm != nullptr && aligned(init, 8) && aligned(Tm, 8) && aligned(active, 4),
                "map_localize_begin: init and T (8-byte aligned) are required%s", "");
  hipLaunchKernelGGL(map_localize_begin_kernel, dim3(ceil_div(S, 64)), dim3(64), 0, current_stream(), S, init, active, Tm);
  check_launch("map_localize_begin");
}

extern "C" void map_localize_accumulate_kernel_wrapper(int S, int n, long long T, int capacity, double voxel, int radius,
                                                       const void *keys, const float *points, const int *source,
                                                       const int *total, int total_stride, const int *index,
                                                       const float *p, const double *pose, const int *max_source_frame,
                                                       double sigma, float max_dist, int min_neighbours, double *partial,
                                                       int *rank, int *count, float *dist, float *normal,
                                                       const int *active) {
  ML_MAP_ARGS("map_localize_accumulate");
  PWCLO_REQUIRE(n >= 1 && (long long)n * 3 < (1ll << 31), "map_localize_accumulate: n=%d out of range", n);
  PWCLO_REQUIRE(radius == 1 || radius == 2, "map_localize_accumulate: radius=%d must be 1 or 2", radius);
  PWCLO_REQUIRE(sigma > 0.0 && isfinite(sigma) && max_dist >= 0.0f && (double)max_dist <= radius * voxel,
                "map_localize_accumulate: sigma=%g must be > 0 and 0 <= max_dist=%.9g <= radius * voxel=%.9g", sigma,
                (double)max_dist, radius * voxel);
  PWCLO_REQUIRE(min_neighbours >= 1, "map_localize_accumulate: min_neighbours=%d must be >= 1", min_neighbours);
  PWCLO_REQUIRE(p != nullptr && partial != nullptr && aligned(p, 4) && aligned(pose, 8) && aligned(partial, 8) &&
                aligned(max_source_frame, 4) && aligned(active, 4),
                "map_localize_accumulate: p and partial (fp64 arrays 8-byte aligned) are required%s", "");
  PWCLO_REQUIRE((rank == nullptr) == (count == nullptr) && (rank == nullptr) == (dist == nullptr) &&
                (rank == nullptr) == (normal == nullptr), "map_localize_accumulate: rank, count, dist and normal come together%s",
                "");
  const dim3 grid(ceil_div(n, ICP_ACC_THREADS), S), block(ICP_ACC_THREADS);
  if (radius == 1)
    hipLaunchKernelGGL(map_localize_accumulate_kernel<1>, grid, block, 0, current_stream(), m, n, p, pose, index,
                       max_source_frame, sigma, max_dist, min_neighbours, partial, rank, count, dist, normal, active);
  else
    hipLaunchKernelGGL(map_localize_accumulate_kernel<2>, grid, block, 0, current_stream(), m, n, p, pose, index,
                       max_source_frame, sigma, max_dist, min_neighbours, partial, rank, count, dist, normal, active);
  check_launch("map_localize_accumulate");
}
