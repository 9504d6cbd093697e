// Layout constants of the loop detector (loop_closure.hip) and the two bin decisions of its
// descriptor.  All bin arithmetic is fp32 in the order tests/loop_closure_model.py evaluates it (the library is built with
// -ffp-contract=off), so that NumPy float32 repeats every decision bit for bit.
#pragma once
#include "common.hpp"

namespace pwclo {

constexpr int LC_MAX_STREAMS = 1024;
constexpr int LC_MAX_RINGS = 64;
constexpr int LC_MIN_SECTORS = 8, LC_MAX_SECTORS = 64;      // one shift per lane of a wave
constexpr int LC_BUILD_THREADS = 256;                       // build: one workgroup per stream
constexpr int LC_SCORE_WAVES = 4;                           // score: one wave per entry, four entries per workgroup
constexpr int LC_SELECT_THREADS = 256;                      // select: one workgroup per stream
constexpr int LC_COPY_THREADS = 256;                        // insert / fetch: grid (LC_COPY_BLOCKS, S)
constexpr int LC_COPY_BLOCKS = 8;
constexpr int LC_MATCH = 4;                                 // the match record's ints: found, entry, frame_i, shift
constexpr int LC_LOG_I = 4;                                 // a log record's ints: i, j, shift, pairs
constexpr int LC_LOG_C = 2;                                 // and its doubles beside T: score, cost
constexpr int LC_ICP_FEW_PAIRS = 2, LC_ICP_BAD_PIVOT = 4;   // the refiner's status bits that refuse a closure (icp.hpp)

__device__ __forceinline__ bool lc_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// Ring of r2 < b[NR - 1]: the number of k in 1..NR-1 with b_k <= r2; b[k - 1] holds b_k.
__device__ __forceinline__ int lc_ring(const float *__restrict__ b, int NR, float r2) {
  int ring = 0;
  for (int k = 0; k < NR - 1; ++k) ring += b[k] <= r2 ? 1 : 0;
  return ring;
}

// Is (x, y) in sector s: dot_s > 0, cross_s >= 0 and cross_{s+1} < 0, with d (NS, 2) the sector directions.
__device__ __forceinline__ bool lc_in_sector(const float *__restrict__ d, int NS, int s, float x, float y) {
  const int t = s + 1 == NS ? 0 : s + 1;
  const float dx = d[2 * s], dy = d[2 * s + 1], ex = d[2 * t], ey = d[2 * t + 1];
  const float cross_s = dx * y - dy * x;
  const float dot_s = dx * x + dy * y;
  const float cross_t = ex * y - ey * x;
  return dot_s > 0.f && cross_s >= 0.f && cross_t < 0.f;
}

// The sector of (x, y), r2 > 0: a guess from atan2f, then the predicate on the guess and its two neighbours to each side
// (the predicate decides, never the angle); every sector is tried where none of the five holds.  -1: no sector holds (a
// point so far out that the products overflow; the caller drops it).
__device__ __forceinline__ int lc_sector(const float *__restrict__ d, int NS, float x, float y) {
  int g = (int)floorf(atan2f(y, x) * (float)NS * 0.15915494309189535f);
  g = ((g % NS) + NS) % NS;
  for (int k = 0; k < 5; ++k) {
    const int c = k == 0 ? g : k == 1 ? g + 1 : k == 2 ? g + NS - 1 : k == 3 ? g + 2 : g + NS - 2;
    const int s = c >= NS ? c - NS : c;
    if (lc_in_sector(d, NS, s, x, y)) return s;
  }
  for (int s = 0; s < NS; ++s)
    if (lc_in_sector(d, NS, s, x, y)) return s;
  return -1;
}

// rot_NS(m, s): bit j of the result is bit (j + s) mod NS of m; 0 <= s < NS <= 64.
__device__ __forceinline__ unsigned long long lc_rotate(unsigned long long m, int NS, int s) {
  const unsigned long long full = NS == 64 ? ~0ull : (1ull << NS) - 1ull;
  return s == 0 ? (m & full) : (((m >> s) | (m << (NS - s))) & full);
}

}  // namespace pwclo
