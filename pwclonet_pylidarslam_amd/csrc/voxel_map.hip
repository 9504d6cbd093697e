// Point-to-plane registration of a frame against a persistent voxel map per stream (gfx950).
//
// registration.IcpRefiner keeps a ring of the last frames and searches every slot in every iteration; this map keeps one
// point per octant of a toroidal voxel grid for as long as the sensor stays near it, and a lookup is a fixed gather of 27
// voxels with no search structure.  voxel_map.hpp holds the coordinate arithmetic, icp.hpp the rows of the normal
// equations; this file holds
//   voxel_begin_kernel       empties the grids of the streams whose frame starts a new sequence
//   voxel_accumulate_kernel  q = fp32(P T p), the nearest stored point among the 27 voxels around q, the row of sums
//   voxel_claim_kernel       insertion, phase 1 and 2: the frame's voxels claim their cells; a stale cell's keys are emptied
//   voxel_min_kernel         insertion, phase 3: 64-bit atomicMin of (seq << 32 | row) on the octant's key
//   voxel_resolve_kernel     insertion, phase 4: the row whose key stands writes its point and normal
//   voxel_pose_kernel        P <- P T, the insertion counter, the nonempty and armed words
// The solver is icp_solve_kernel, unchanged.  The only read-modify-write atomic is the 64-bit min, whose result does not
// depend on the order of arrival; coordinate words are touched by 64-bit relaxed atomic loads and stores only, and all
// writers of a word within one launch write the same value.  No loop bound depends on data, nothing spins or waits, and
// every sum is added in a fixed order: two runs give the same bits and a captured graph serves every frame.
//
// Masks: every kernel takes a nullable `active` (S) of device words; nullptr is lock step.  A stream with active[s] == 0 is
// idle: its grid, P, seq, nonempty and T keep their bits and its rows of sums are zero.  The word is the same for a whole
// workgroup (blockIdx.y -> s), so the exit is uniform.
#include <math.h>

#include "common.hpp"
#include "voxel_map.hpp"

namespace pwclo {

constexpr int VM_BEGIN_WORDS = 4096;        // coordinate words one workgroup of voxel_begin_kernel empties

struct VmGrid {
  int nx, ny, nz;
  double voxel, half;
  unsigned long long *coord, *keys;         // this launch's sections, all streams
  float *pts, *nrm;
  __device__ __forceinline__ size_t cells() const { return (size_t)nx * ny * nz; }
};

__device__ __forceinline__ unsigned long long vm_load(const unsigned long long *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void vm_store(unsigned long long *p, unsigned long long v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One workgroup per VM_BEGIN_WORDS coordinate words of a stream.  active: (S) or nullptr (all); restart, armed: (S) or
// nullptr (none).  armed is only read here (every workgroup of the stream reads it); voxel_pose_kernel clears it.
__global__ __launch_bounds__(256) void voxel_begin_kernel(VmGrid g, const int *__restrict__ active,
                                                          const int *__restrict__ restart, const int *__restrict__ armed,
                                                          double *__restrict__ P, int *__restrict__ nonempty,
                                                          int *__restrict__ seq) {
  const int s = blockIdx.y;
  if (active != nullptr && active[s] == 0) return;
  const bool clear = (restart != nullptr && restart[s] != 0) || (armed != nullptr && armed[s] != 0);
  if (!clear) return;
  const size_t cells = g.cells();
  unsigned long long *c = g.coord + (size_t)s * cells;
#pragma unroll 4
  for (int r = 0; r < VM_BEGIN_WORDS / 256; ++r) {
    const size_t j = (size_t)blockIdx.x * VM_BEGIN_WORDS + (size_t)r * 256 + threadIdx.x;
    if (j < cells) vm_store(c + j, VM_EMPTY);
  }
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0) se3_store(P + (size_t)s * 16, se3_identity());
    if (threadIdx.x == 16) nonempty[s] = 0;
    if (threadIdx.x == 17) seq[s] = 0;
  }
}

// The pose a frame is inserted with: I for a stream whose map is empty (nonempty given and zero), else P[s] T[s] (T given)
// or P[s].
__device__ __forceinline__ Se3 vm_insert_pose(int s, const double *__restrict__ P, const double *__restrict__ T,
                                              const int *__restrict__ nonempty) {
  if (nonempty != nullptr && nonempty[s] == 0) return se3_identity();
  const Se3 a = se3_load(P + (size_t)s * 16);
  return T != nullptr ? se3_mul(a, se3_load(T + (size_t)s * 16)) : a;
}

// w = fp32(W p); -> the slot (cell * 8 + octant) the point asks for, -1 when it is not inserted; want: its voxel's word.
__device__ __forceinline__ int vm_insert_slot(const VmGrid &g, const Se3 &W, const float p[3], float w[3],
                                              unsigned long long *want) {
  double o[3];
  se3_apply(W, p, o);
  w[0] = (float)o[0]; w[1] = (float)o[1]; w[2] = (float)o[2];
  if (!(vm_finite(w[0]) && vm_finite(w[1]) && vm_finite(w[2]))) return -1;
  const int N[3] = {g.nx, g.ny, g.nz};
  int h[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!(fabs((double)w[a] - W.m[4 * a + 3]) < (double)(N[a] / 2 - 1) * g.voxel)) return -1;
    if (!vm_half_index(w[a], g.half, &h[a])) return -1;
  }
  const int cx = h[0] >> 1, cy = h[1] >> 1, cz = h[2] >> 1;
  *want = vm_pack(cx, cy, cz);
  const int cell = (vm_mod(cz, g.nz) * g.ny + vm_mod(cy, g.ny)) * g.nx + vm_mod(cx, g.nx);
  return cell * VM_OCTANTS + (((h[2] & 1) << 2) | ((h[1] & 1) << 1) | (h[0] & 1));
}

__device__ __forceinline__ bool vm_inserts(int s, const int *__restrict__ active, const int *__restrict__ insert) {
  if (active != nullptr && active[s] == 0) return false;
  return insert == nullptr || insert[s] != 0;
}

// cloud (S, n, 3) -> slot (S, n).  A cell whose word differs from the voxel that needs it is stale: the word is replaced
// and its eight keys are emptied.  Two voxels of one frame never share a cell (the box rule), so all writers of a word
// write the same value, and nothing reads a key in this launch.
__global__ __launch_bounds__(256) void voxel_claim_kernel(VmGrid g, int n, const float *__restrict__ cloud,
                                                          const double *__restrict__ P, const double *__restrict__ T,
                                                          const int *__restrict__ nonempty, int *__restrict__ slot,
                                                          const int *__restrict__ active, const int *__restrict__ insert) {
  const int s = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (!vm_inserts(s, active, insert)) return;
  if (i >= n) return;
  const Se3 W = vm_insert_pose(s, P, T, nonempty);
  const float *pr = cloud + ((size_t)s * n + i) * 3;
  const float p[3] = {pr[0], pr[1], pr[2]};
  float w[3];
  unsigned long long want = VM_EMPTY;
  const int sl = vm_insert_slot(g, W, p, w, &want);
  slot[(size_t)s * n + i] = sl;
  if (sl < 0) return;
  const size_t cell = (size_t)s * g.cells() + (size_t)(sl >> 3);
  if (vm_load(g.coord + cell) != want) {
    vm_store(g.coord + cell, want);
#pragma unroll
    for (int o = 0; o < VM_OCTANTS; ++o) g.keys[cell * VM_OCTANTS + o] = VM_EMPTY;
  }
}

// The first point ever to reach an octant stays: an earlier seq beats a later one, within a frame the lowest row wins.
__global__ __launch_bounds__(256) void voxel_min_kernel(VmGrid g, int n, const int *__restrict__ slot,
                                                        const int *__restrict__ seq, const int *__restrict__ active,
                                                        const int *__restrict__ insert) {
  const int s = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (!vm_inserts(s, active, insert)) return;
  if (i >= n) return;
  const int sl = slot[(size_t)s * n + i];
  if (sl < 0) return;
  const unsigned long long key = ((unsigned long long)(unsigned)seq[s] << 32) | (unsigned)i;
  atomicMin(g.keys + (size_t)s * g.cells() * VM_OCTANTS + (size_t)sl, key);
}

__global__ __launch_bounds__(256) void voxel_resolve_kernel(VmGrid g, int n, const float *__restrict__ cloud,
                                                            const float *__restrict__ normals,
                                                            const double *__restrict__ P, const double *__restrict__ T,
                                                            const int *__restrict__ nonempty, const int *__restrict__ slot,
                                                            const int *__restrict__ seq, const int *__restrict__ active,
                                                            const int *__restrict__ insert) {
  const int s = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (!vm_inserts(s, active, insert)) return;
  if (i >= n) return;
  const int sl = slot[(size_t)s * n + i];
  if (sl < 0) return;
  const size_t e = (size_t)s * g.cells() * VM_OCTANTS + (size_t)sl;
  const unsigned long long key = ((unsigned long long)(unsigned)seq[s] << 32) | (unsigned)i;
  if (g.keys[e] != key) return;
  const Se3 W = vm_insert_pose(s, P, T, nonempty);
  const float *pr = cloud + ((size_t)s * n + i) * 3, *nr = normals + ((size_t)s * n + i) * 3;
  const float p[3] = {pr[0], pr[1], pr[2]};
  const double nd[3] = {nr[0], nr[1], nr[2]};
  double o[3], on[3];
  se3_apply(W, p, o);
  se3_rotate(W, nd, on);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    g.pts[e * 3 + a] = (float)o[a];
    g.nrm[e * 3 + a] = (float)on[a];
  }
}

// One workgroup, one thread per stream, after the insertion's launches (which read the old words).  A stream whose map was
// empty gets P = I, any other P <- P T (T given); a stream that inserted counts the frame and owns a map from now on; the
// restart that reset() armed has been consumed by this frame.
__global__ __launch_bounds__(VM_MAX_STREAMS) void voxel_pose_kernel(int S, const double *__restrict__ T,
                                                                    double *__restrict__ P, int *__restrict__ nonempty,
                                                                    int *__restrict__ seq, int *__restrict__ armed,
                                                                    const int *__restrict__ active,
                                                                    const int *__restrict__ insert) {
  const int s = threadIdx.x;
  if (s >= S) return;
  if (active != nullptr && active[s] == 0) return;
  se3_store_rows(P + (size_t)s * 16, vm_insert_pose(s, P, T, nonempty));
  if (insert == nullptr || insert[s] != 0) {
    seq[s] += 1;
    nonempty[s] = 1;
  }
  if (armed != nullptr) armed[s] = 0;
}

// p (S, n, 3), P (S, 4, 4), T (S, 4, 4) or nullptr (the identity) -> partial (S, gridDim.x, ICP_ROW) in icp_solve_kernel's
// layout.  cell / octant / dist: (S, n) or nullptr, the nearest candidate of every point whatever became of the pair (-1,
// -1, +Inf where there is none).
__global__ __launch_bounds__(ICP_ACC_THREADS) void voxel_accumulate_kernel(
    VmGrid g, int n, const float *__restrict__ p, const double *__restrict__ P, const double *__restrict__ T, double sigma,
    float max_dist, double *__restrict__ partial, int *__restrict__ cell_out, int *__restrict__ octant_out,
    float *__restrict__ dist_out, const int *__restrict__ active) {
  const int s = blockIdx.y, i = blockIdx.x * ICP_ACC_THREADS + threadIdx.x;
  if (active != nullptr && active[s] == 0) {              // idle: a zero row, no gather (the whole workgroup leaves)
    icp_store_zero_row(partial, s);
    return;
  }
  double acc[ICP_TERMS];
#pragma unroll
  for (int e = 0; e < ICP_TERMS; ++e) acc[e] = 0.0;
  if (i < n) {
    const Se3 a = se3_load(P + (size_t)s * 16), t = T != nullptr ? se3_load(T + (size_t)s * 16) : se3_identity();
    const Se3 W = se3_mul(a, t);
    const float *pr = p + ((size_t)s * n + i) * 3;
    const float pp[3] = {pr[0], pr[1], pr[2]};
    double o[3];
    se3_apply(W, pp, o);
    const float q[3] = {(float)o[0], (float)o[1], (float)o[2]};
    int best = -1;
    float bd = INFINITY;
    int h[3];
    if (vm_half_index(q[0], g.half, &h[0]) && vm_half_index(q[1], g.half, &h[1]) && vm_half_index(q[2], g.half, &h[2])) {
      const int c[3] = {h[0] >> 1, h[1] >> 1, h[2] >> 1};
      const size_t cells = g.cells();
      const unsigned long long *coord = g.coord + (size_t)s * cells, *keys = g.keys + (size_t)s * cells * VM_OCTANTS;
      const float *pts = g.pts + (size_t)s * cells * VM_OCTANTS * 3;
#pragma unroll 1
      for (int dz = -1; dz <= 1; ++dz) {
        const int cz = c[2] + dz, mz = vm_mod(cz, g.nz);
#pragma unroll 1
        for (int dy = -1; dy <= 1; ++dy) {
          const int cy = c[1] + dy, my = vm_mod(cy, g.ny);
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {
            const int cx = c[0] + dx;
            if (!(vm_voxel_in_range(cx) && vm_voxel_in_range(cy) && vm_voxel_in_range(cz))) continue;
            const int cell = (mz * g.ny + my) * g.nx + vm_mod(cx, g.nx);
            if (vm_load(coord + cell) != vm_pack(cx, cy, cz)) continue;      // empty, or a voxel that aliases onto the cell
#pragma unroll
            for (int oc = 0; oc < VM_OCTANTS; ++oc) {
              const int e = cell * VM_OCTANTS + oc;
              if (keys[e] == VM_EMPTY) continue;
              const float ex = q[0] - pts[(size_t)e * 3], ey = q[1] - pts[(size_t)e * 3 + 1], ez = q[2] - pts[(size_t)e * 3 + 2];
              const float d = sqrtf((ex * ex + ey * ey) + ez * ez);
              if (best < 0 || d < bd) {                     // strict: the first candidate stays on a tie
                best = e;
                bd = d;
              }
            }
          }
        }
      }
      if (best >= 0 && bd <= max_dist) {                    // NaN fails
        const float *yr = pts + (size_t)best * 3, *nr = g.nrm + ((size_t)s * cells * VM_OCTANTS + best) * 3;
        const float y[3] = {yr[0], yr[1], yr[2]}, nn[3] = {nr[0], nr[1], nr[2]};
        if (nn[0] != 0.0f || nn[1] != 0.0f || nn[2] != 0.0f) {
          double r9[9];
#pragma unroll
          for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) r9[3 * r + cc] = a.m[4 * cc + r];       // R_P^T: the map frame -> the previous frame
          icp_add_pair(pp, q, y, nn, t, r9, sigma, acc);
        }
      }
    }
    if (cell_out != nullptr) {
      cell_out[(size_t)s * n + i] = best < 0 ? -1 : best >> 3;
      octant_out[(size_t)s * n + i] = best < 0 ? -1 : best & 7;
      dist_out[(size_t)s * n + i] = bd;
    }
  }
  icp_reduce_store_row(acc, partial, s);
}

}  // namespace pwclo

using namespace pwclo;

static bool vm_extent_ok(int S, int nx, int ny, int nz) {
  const int N[3] = {nx, ny, nz};
  for (int a = 0; a < 3; ++a)
    if (N[a] < 4 || N[a] > VM_MAX_AXIS || (N[a] & 1)) return false;
  return S >= 1 && S <= VM_MAX_STREAMS && (long long)nx * ny * nz * VM_OCTANTS < (1ll << 31);
}

extern "C" long long voxel_map_bytes(int S, int nx, int ny, int nz) {
  return vm_extent_ok(S, nx, ny, nz) ? (long long)S * nx * ny * nz * VM_CELL_BYTES : 0;
}

static VmGrid vm_grid(int S, int nx, int ny, int nz, double voxel, void *grid) {
  const size_t cells = (size_t)nx * ny * nz;
  char *base = static_cast<char *>(grid);
  VmGrid g;
  g.nx = nx; g.ny = ny; g.nz = nz;
  g.voxel = voxel; g.half = voxel / 2;
  g.coord = reinterpret_cast<unsigned long long *>(base);
  g.keys = reinterpret_cast<unsigned long long *>(base + vm_keys_offset(S, cells));
  g.pts = reinterpret_cast<float *>(base + vm_points_offset(S, cells));
  g.nrm = reinterpret_cast<float *>(base + vm_normals_offset(S, cells));
  return g;
}

#define VM_REQUIRE_GRID(what)                                                                                          \
  PWCLO_REQUIRE(vm_extent_ok(S, nx, ny, nz), "%s: S=%d extent=(%d, %d, %d) out of range (S <= %d; even, 4 <= N <= %d, "  \
                "Nx Ny Nz < 2^28)", what, S, nx, ny, nz, VM_MAX_STREAMS, VM_MAX_AXIS);                                  \
  PWCLO_REQUIRE(voxel > 0.0 && isfinite(voxel), "%s: voxel_size=%g must be finite and > 0", what, voxel);              \
  PWCLO_REQUIRE(grid != nullptr && aligned(grid, 8), "%s: the grid (8-byte aligned) is required", what)

extern "C" void voxel_begin_kernel_wrapper(int S, int nx, int ny, int nz, const int *active, const int *restart,
                                           const int *armed, void *grid, double *P, int *nonempty, int *seq) {
  if (S <= 0) return;
  const double voxel = 1.0;
  VM_REQUIRE_GRID("voxel_begin");
  PWCLO_REQUIRE(P != nullptr && nonempty != nullptr && seq != nullptr && aligned(P, 8),
                "voxel_begin: P (8-byte aligned), nonempty and seq are required%s", "");
  PWCLO_REQUIRE(aligned(active, 4) && aligned(restart, 4) && aligned(armed, 4),
                "voxel_begin: mask words must be 4-byte aligned%s", "");
  const VmGrid g = vm_grid(S, nx, ny, nz, voxel, grid);
  const long long cells = (long long)nx * ny * nz;
  hipLaunchKernelGGL(voxel_begin_kernel, dim3((unsigned)((cells + VM_BEGIN_WORDS - 1) / VM_BEGIN_WORDS), S), dim3(256), 0,
                     current_stream(), g, active, restart, armed, P, nonempty, seq);
  check_launch("voxel_begin");
}

extern "C" void voxel_insert_kernel_wrapper(int S, int n, int nx, int ny, int nz, double voxel, const float *cloud,
                                            const float *normals, const double *P, const double *T, const int *nonempty,
                                            const int *seq, void *grid, int *slot, const int *active, const int *insert) {
  if (S <= 0) return;
  VM_REQUIRE_GRID("voxel_insert");
  PWCLO_REQUIRE(n >= 1 && (long long)n * 3 < (1ll << 31), "voxel_insert: n=%d out of range", n);
  PWCLO_REQUIRE(cloud != nullptr && normals != nullptr && P != nullptr && seq != nullptr && slot != nullptr,
                "voxel_insert: cloud, normals, P, seq and slot are required%s", "");
  PWCLO_REQUIRE(aligned(P, 8) && aligned(T, 8) && aligned(active, 4) && aligned(insert, 4),
                "voxel_insert: fp64 arrays must be 8-byte, mask words 4-byte aligned%s", "");
  const VmGrid g = vm_grid(S, nx, ny, nz, voxel, grid);
  const dim3 blocks(ceil_div(n, 256), S);
  hipLaunchKernelGGL(voxel_claim_kernel, blocks, dim3(256), 0, current_stream(), g, n, cloud, P, T, nonempty, slot, active,
                     insert);
  hipLaunchKernelGGL(voxel_min_kernel, blocks, dim3(256), 0, current_stream(), g, n, slot, seq, active, insert);
  hipLaunchKernelGGL(voxel_resolve_kernel, blocks, dim3(256), 0, current_stream(), g, n, cloud, normals, P, T, nonempty, slot,
                     seq, active, insert);
  check_launch("voxel_insert");
}

extern "C" void voxel_pose_kernel_wrapper(int S, const double *T, double *P, int *nonempty, int *seq, int *armed,
                                          const int *active, const int *insert) {
  if (S <= 0) return;
  PWCLO_REQUIRE(S <= VM_MAX_STREAMS, "voxel_pose: S=%d out of range (S <= %d)", S, VM_MAX_STREAMS);
  PWCLO_REQUIRE(P != nullptr && nonempty != nullptr && seq != nullptr && aligned(P, 8) && aligned(T, 8),
                "voxel_pose: P (8-byte aligned), nonempty and seq are required%s", "");
  hipLaunchKernelGGL(voxel_pose_kernel, dim3(1), dim3(ceil_div(S, 64) * 64), 0, current_stream(), S, T, P, nonempty, seq,
                     armed, active, insert);
  check_launch("voxel_pose");
}

extern "C" void voxel_accumulate_kernel_wrapper(int S, int n, int nx, int ny, int nz, double voxel, const float *p,
                                                const double *P, const double *T, const void *grid, double sigma,
                                                float max_dist, double *partial, int *cell, int *octant, float *dist,
                                                const int *active) {
  if (S <= 0) return;
  VM_REQUIRE_GRID("voxel_accumulate");
  PWCLO_REQUIRE(n >= 1 && (long long)n * 3 < (1ll << 31), "voxel_accumulate: n=%d out of range", n);
  PWCLO_REQUIRE(sigma > 0.0 && isfinite(sigma) && max_dist >= 0.0f && (double)max_dist <= voxel,
                "voxel_accumulate: sigma=%g must be > 0 and 0 <= max_dist=%g <= voxel_size=%g", sigma, (double)max_dist,
                voxel);
  PWCLO_REQUIRE(p != nullptr && P != nullptr && partial != nullptr && aligned(P, 8) && aligned(T, 8) &&
                aligned(partial, 8), "voxel_accumulate: p, P and partial (fp64 arrays 8-byte aligned) are required%s", "");
  PWCLO_REQUIRE((cell == nullptr) == (octant == nullptr) && (cell == nullptr) == (dist == nullptr),
                "voxel_accumulate: cell, octant and dist come together%s", "");
  const VmGrid g = vm_grid(S, nx, ny, nz, voxel, const_cast<void *>(grid));
  hipLaunchKernelGGL(voxel_accumulate_kernel, dim3(ceil_div(n, ICP_ACC_THREADS), S), dim3(ICP_ACC_THREADS), 0,
                     current_stream(), g, n, p, P, T, sigma, max_dist, partial, cell, octant, dist, active);
  check_launch("voxel_accumulate");
}
