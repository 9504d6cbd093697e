// The open-addressing table of the voxel grid, shared by every kernel that grid-samples: the
// stand-alone op and the fused front ends of grid_sample.hip, and the de-skewing front end of deskew.hip.  One definition
// of the key, the layout and the three phases (clear, insert, resolve), so all of them choose the same winners.
#pragma once
#include <math.h>

#include "common.hpp"

namespace pwclo {

constexpr unsigned long long GRID_EMPTY = ~0ull;
constexpr int GRID_MAX_ROWS = 1 << 20;          // rows per cloud: keeps the table (2^21 slots at most) far inside int indices

// L with 2^L the table size of a cloud of n rows: the smallest power of two >= 2 n, at least 64 slots.
__host__ __device__ static inline int grid_table_log2(int n) {
  int L = 6;
  while ((1ll << L) < 2ll * n) ++L;
  return L;
}

// One cloud's slice of the workspace, sized by the row capacity n: T keys (8 bytes each), T + 2 row words (the special
// key's word and one word of padding: the clear writes 8 bytes at a time), n slot words.  All offsets are multiples of 8.
struct GridLayout {
  long long rows_off, slots_off, stride;
};
__host__ __device__ static inline GridLayout grid_layout(int n) {
  const long long T = 1ll << grid_table_log2(n);
  GridLayout g;
  g.rows_off = 8 * T;
  g.slots_off = g.rows_off + 4 * (T + 2);
  g.stride = g.slots_off + 4 * (((long long)n + 3) & ~3ll);
  return g;
}

static inline bool grid_voxel_ok(double voxel) { return voxel > 0.0 && isfinite(voxel); }

#if defined(__HIPCC__)

struct GridTable {
  unsigned long long *keys;
  unsigned *rows;
  int log2T;
};

__device__ __forceinline__ void grid_phase_barrier() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's stores and atomics have been performed
  __syncthreads();
}

__device__ __forceinline__ void grid_clear(const GridTable t) {
  const int T = 1 << t.log2T;
  for (int j = threadIdx.x; j < T; j += blockDim.x)
    __hip_atomic_store(t.keys + j, GRID_EMPTY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  unsigned long long *r2 = reinterpret_cast<unsigned long long *>(t.rows);
  for (int j = threadIdx.x; j < T / 2 + 1; j += blockDim.x)
    __hip_atomic_store(r2 + j, ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The voxel hash of one point; false: the row is no candidate (rule 4).
__device__ __forceinline__ bool grid_key(const float o[3], double voxel, unsigned long long &h) {
  bool ok = true;
  long long q[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double d = (double)o[a] / voxel;
    const bool in = fabs(d) < 2147483648.0;              // false for NaN and for +-inf
    ok = ok && in;
    q[a] = (long long)rint(in ? d : 0.0);
  }
  h = 73856093ull * (unsigned long long)q[0] + 19349669ull * (unsigned long long)q[1] + 83492791ull * (unsigned long long)q[2];
  return ok;
}

// Enters (h, row i) and returns the slot that now holds h.  The table has at least twice as many slots as rows, so a
// probe sequence always meets an empty slot or its own key.
__device__ __forceinline__ int grid_insert(const GridTable t, unsigned long long h, unsigned i) {
  const int T = 1 << t.log2T;
  int slot = T;                                          // the empty marker's own row word
  if (h != GRID_EMPTY) {
    slot = (int)((h * 0x9E3779B97F4A7C15ull) >> (64 - t.log2T));
    for (;;) {
      unsigned long long cur = __hip_atomic_load(t.keys + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == GRID_EMPTY) {
        unsigned long long expected = GRID_EMPTY;
        const bool won = __hip_atomic_compare_exchange_strong(t.keys + slot, &expected, h, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                              __HIP_MEMORY_SCOPE_AGENT);
        cur = won ? h : expected;
      }
      if (cur == h) break;
      slot = (slot + 1) & (T - 1);
    }
  }
  __hip_atomic_fetch_min(t.rows + slot, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return slot;
}

__device__ __forceinline__ bool grid_is_winner(const GridTable t, int slot, unsigned i) {
  return __hip_atomic_load(t.rows + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == i;
}

__device__ __forceinline__ GridTable grid_table(char *ws, int cloud, int capacity_rows, int n) {
  const GridLayout g = grid_layout(capacity_rows);
  char *base = ws + (long long)cloud * g.stride;
  return GridTable{reinterpret_cast<unsigned long long *>(base), reinterpret_cast<unsigned *>(base + g.rows_off),
                   grid_table_log2(n)};
}

#endif  // __HIPCC__

}  // namespace pwclo
