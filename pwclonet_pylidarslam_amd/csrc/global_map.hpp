// The global map of a stream: sizes, limits and the words of its state, shared by the kernels and
// the host checks of global_map.hip.  The table is grid.hpp's, sized once by the bank's capacity MK * n rows.
#pragma once
#include "grid.hpp"

namespace pwclo {

constexpr int GM_MAX_STREAMS = 1024;
constexpr int GM_MAX_KEYFRAMES = 65535;          // a keyframe is one blockIdx.y of the insert / count / write grids
constexpr int GM_MAX_ROWS = 1 << 29;             // MK * n: a global row id and a table of 2^30 slots fit an int
constexpr int GM_BLOCK = 256;                    // rows per workgroup: four waves, never more than one keyframe

// The state words of a stream, (S, 8) ints.
enum GmWord : int {
  GM_COUNT = 0,      // keyframes in the bank
  GM_BUILT = 1,      // keyframes [0, built) are in the table and in the map
  GM_TOTAL = 2,      // winners so far, not clamped
  GM_DIRTY = 3,      // the table holds keys of a bank that is gone, or of other poses: clear before the next insert
  GM_TODO = 4,       // keyframes [built, built + todo) are this call's
  GM_SLOT = 5,       // the bank slot this call's frame goes to, -1: none
  GM_RUN = 6,        // this call touches the stream (an idle stream keeps every word)
  GM_WORDS = 8
};

__host__ __device__ static inline int gm_blocks(int n) { return (n + GM_BLOCK - 1) / GM_BLOCK; }
__host__ __device__ static inline int gm_table_log2(int MK, int n) { return grid_table_log2(MK * n); }

static inline bool gm_sizes_ok(int S, int MK, int n) {
  return S >= 1 && S <= GM_MAX_STREAMS && MK >= 1 && MK <= GM_MAX_KEYFRAMES && n >= 1 &&
         (long long)MK * n <= (long long)GM_MAX_ROWS;
}

}  // namespace pwclo
