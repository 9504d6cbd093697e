// Arithmetic of the persistent voxel map, shared by the kernels of voxel_map.hip and by host code that
// wants the same numbers (the pattern of icp.hpp, grid.hpp and deskew.hpp).
//
// A stream's map is a toroidal grid of Nx x Ny x Nz voxels of edge `voxel`: voxel c = (cx, cy, cz) lives in cell (cx mod Nx,
// cy mod Ny, cz mod Nz) (floor-mod), cell index (mz * Ny + my) * Nx + mx.  A cell holds the packed coordinate of the voxel
// that owns it and eight entries, one per octant of edge voxel / 2.  Every coordinate goes through one expression:
//   h_a = floor((double)w_a / (voxel / 2)),  voxel c_a = h_a >> 1,  octant bit a = h_a & 1,  octant = bz << 2 | by << 1 | bx
// A coordinate packs into 21 bits per axis with bias 2^20, so a point is storable only where -2^21 <= h_a < 2^21 on every
// axis; all ones is the empty word, which no packed coordinate equals (bit 63 is never set).
#pragma once
#include "icp.hpp"

namespace pwclo {

constexpr unsigned long long VM_EMPTY = ~0ull;      // an empty coordinate word, an empty key
constexpr int VM_BIAS = 1 << 20;
constexpr int VM_OCTANTS = 8;
constexpr int VM_CELL_BYTES = 8 + 8 * (8 + 12 + 12);   // coordinate, then per octant: key, point, normal = 264
constexpr int VM_MAX_AXIS = 1024;                   // voxels per axis, and Nx * Ny * Nz * 8 < 2^31
constexpr int VM_MAX_STREAMS = 1024;

// h = floor((double)w / half) where it is in range; NaN and +-Inf are out of range.
ICP_HD bool vm_half_index(float w, double half, int *h) {
  const double f = floor((double)w / half);
  if (!(f >= -2097152.0 && f < 2097152.0)) return false;
  *h = (int)f;
  return true;
}
ICP_HD bool vm_voxel_in_range(int c) { return c >= -VM_BIAS && c < VM_BIAS; }
ICP_HD unsigned long long vm_pack(int cx, int cy, int cz) {
  return ((unsigned long long)(unsigned)(cz + VM_BIAS) << 42) | ((unsigned long long)(unsigned)(cy + VM_BIAS) << 21) |
         (unsigned long long)(unsigned)(cx + VM_BIAS);
}
ICP_HD int vm_mod(int c, int n) {
  const int m = c % n;
  return m < 0 ? m + n : m;
}
ICP_HD bool vm_finite(float v) { return v - v == 0.0f; }   // false for NaN and +-Inf

// Where a stream's four sections start inside the grid buffer, in bytes: coordinates (S, cells) u64, keys (S, cells, 8) u64,
// points (S, cells, 8, 3) fp32, normals (S, cells, 8, 3) fp32.
ICP_HD size_t vm_keys_offset(size_t S, size_t cells) { return S * cells * 8; }
ICP_HD size_t vm_points_offset(size_t S, size_t cells) { return S * cells * (8 + 64); }
ICP_HD size_t vm_normals_offset(size_t S, size_t cells) { return S * cells * (8 + 64 + 96); }

}  // namespace pwclo
