// Layout constants of the loop detector's translation search (elevation.hip) and the cell decision of
// its elevation grids.  The grid arithmetic is fp32 in the order tests/elevation_model.py evaluates it (the library is built
// with -ffp-contract=off), so that NumPy float32 repeats every decision bit for bit; every score is an integer sum.
#pragma once
#include "loop_closure.hpp"

namespace pwclo {

constexpr int EL_MIN_CELLS = 8, EL_MAX_CELLS = 128;         // G, even
constexpr int EL_MAX_WINDOW = 16;                           // W: offsets a, b in [-W, W]
constexpr int EL_MAX_YAW = 17;                              // Y = 2 Yh + 1, Yh <= 8
constexpr int EL_IMAGE_THREADS = 256;                       // image: grid (1 + Y, S)
constexpr int EL_SCORE_WAVES = 4;                           // score: one wave per 64 candidates of one (stream, k)
constexpr int EL_CHOOSE_THREADS = 256;                      // choose: one workgroup per stream
constexpr int EL_RECORD = 8;                                // found, k, a, b, A, occ_Q, occ_E, (unused)

// The cell and the level of a row (x, y, z) in the descriptor's axes under the planar rotation (cs, sn): false where the
// row is dropped.  fx and fy are compared as floats before any conversion, so NaN and overflow never reach an index.
__device__ __forceinline__ bool el_cell(float x, float y, float z, float cs, float sn, float c, float zs, float z_offset, int G,
                                        int &i, int &j, int &q) {
  const float xr = cs * x - sn * y;
  const float yr = sn * x + cs * y;
  const float fx = floorf(xr / c);
  const float fy = floorf(yr / c);
  const float h = z + z_offset;
  const float half = (float)(G / 2);
  if (!(fx >= -half && fx < half && fy >= -half && fy < half)) return false;
  if (!(h > 0.f)) return false;
  const float l = floorf(h / zs);
  q = l >= 254.f ? 255 : (int)l + 1;
  i = (int)fx + G / 2;
  j = (int)fy + G / 2;
  return true;
}

}  // namespace pwclo
