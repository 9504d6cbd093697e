// The global map on the device (gfx950): per stream a bank of keyframe clouds and the voxel-hashed
// map of their rows at given poses, one row per occupied voxel: the lowest global row id g = k n + i.
//
// The rule is section 19's with the row's world point in the place of the row:
//   w   = float32(se3_apply(X[bank_frame[k]], p))      fp64, unfused, one rounding
//   h   = grid_key(w, v)                               fp64 division, rint, the 64-bit hash; no candidate where it says so
//   row g is a winner iff no candidate row of the stream with a lower g has the same h
// and the map is the winners' w in ascending g.  grid.hpp's table does the deduplication, here across many workgroups
// and launches: the table is sized once for the whole bank (T >= 2 MK n slots), so a later call enters its rows beside
// the earlier ones without clearing, and the row word's minimum keeps the older row: with unchanged poses a new keyframe
// can only append.  The phases that depend on each other grid-wide are separate launches:
//   begin   one thread per stream: restart, the bank slot of this call's frame, todo
//   push    the frame's rows into the bank slot
//   clear   the tables of the streams with the dirty word (restart, reset, rebuild)
//   insert  grid (ceil(n / 256), E, S): 256 rows of keyframe built + blockIdx.y: world point, key, grid_insert, the slot
//           parked in the row's slot word
//   count   per workgroup the winners among its rows (ballot, popcount, LDS over the four waves)
//   scan    one workgroup per stream: exclusive scan of the block counts in block order on top of the old total
//   write   the winners again, ranked in-wave, w recomputed by the same body (the same bits), written below capacity
//   end     built += todo, dirty = 0
// Every table access in the insert launch is grid.hpp's relaxed agent-scope atomic; nothing spins on another workgroup.
#include <math.h>

#include "common.hpp"
#include "global_map.hpp"
#include "grid.hpp"
#include "se3.hpp"

namespace pwclo {

__device__ __forceinline__ GridTable gm_table(unsigned long long *keys, unsigned *rows, int s, int log2T) {
  const long long T = 1ll << log2T;
  return GridTable{keys + (long long)s * T, rows + (long long)s * (T + 2), log2T};
}

// The world point of row i of keyframe k, rounded once; false where the keyframe's frame id has no pose.
__device__ __forceinline__ bool gm_world(const double *__restrict__ X, int frames, int S, int s, int frame,
                                         const float *__restrict__ p, float w[3]) {
  if (frame < 0 || frame >= frames) return false;
  const Se3 a = se3_load(X + ((size_t)frame * S + s) * 16);
  const float q[3] = {p[0], p[1], p[2]};
  double o[3];
  se3_apply(a, q, o);
  w[0] = (float)o[0];
  w[1] = (float)o[1];
  w[2] = (float)o[2];
  return true;
}

// mode 0: a streaming call (active / restart / frame_id / lengths are the call's), mode 1: a rebuild of every stream.
__global__ void gm_begin_kernel(int S, int MK, int n, int stride, int E, int mode, const int *__restrict__ active,
                                const int *__restrict__ restart, const int *__restrict__ frame_id,
                                const int *__restrict__ lengths, int *__restrict__ state, int *__restrict__ bank_frame,
                                int *__restrict__ bank_len, int *__restrict__ overflow) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  int *st = state + (size_t)s * GM_WORDS;
  const bool run = mode == 1 || active == nullptr || active[s] != 0;
  st[GM_RUN] = run ? 1 : 0;
  st[GM_SLOT] = -1;
  st[GM_TODO] = 0;
  if (!run) return;
  int count = st[GM_COUNT], built = st[GM_BUILT];
  if (mode == 1) {
    built = 0;
    st[GM_TOTAL] = 0;
    st[GM_DIRTY] = 1;
  } else {
    if (restart != nullptr && restart[s] != 0) {
      count = built = 0;
      st[GM_TOTAL] = 0;
      st[GM_DIRTY] = 1;
    }
    const int f = frame_id[s];
    if (f >= 0 && f % stride == 0) {
      if (count < MK) {
        const int len = lengths ? min(max(lengths[s], 0), n) : n;
        bank_frame[(size_t)s * MK + count] = f;
        bank_len[(size_t)s * MK + count] = len;
        st[GM_SLOT] = count;
        ++count;
      } else {
        *overflow = 1;
      }
    }
  }
  st[GM_COUNT] = count;
  st[GM_BUILT] = built;
  st[GM_TODO] = min(count - built, E);
}

__global__ __launch_bounds__(GM_BLOCK) void gm_push_kernel(int MK, int n, const float *__restrict__ cloud,
                                                           const int *__restrict__ state, float *__restrict__ bank_cloud) {
  const int s = blockIdx.y;
  const int slot = state[(size_t)s * GM_WORDS + GM_SLOT];
  if (slot < 0 || slot >= MK) return;
  const int i = blockIdx.x * GM_BLOCK + threadIdx.x;
  if (i >= n) return;
  const float *src = cloud + ((size_t)s * n + i) * 3;
  float *dst = bank_cloud + (((size_t)s * MK + slot) * n + i) * 3;
  dst[0] = src[0];
  dst[1] = src[1];
  dst[2] = src[2];
}

// Grid (blocks, S): a grid-stride loop over the stream's key slots and row words, for the dirty streams only.
__global__ __launch_bounds__(GM_BLOCK) void gm_clear_kernel(int log2T, const int *__restrict__ state,
                                                            unsigned long long *__restrict__ keys,
                                                            unsigned *__restrict__ rows) {
  const int s = blockIdx.y;
  const int *st = state + (size_t)s * GM_WORDS;
  if (st[GM_RUN] == 0 || st[GM_DIRTY] == 0) return;
  const GridTable t = gm_table(keys, rows, s, log2T);
  const long long T = 1ll << log2T;
  const long long step = (long long)gridDim.x * GM_BLOCK;
  for (long long j = (long long)blockIdx.x * GM_BLOCK + threadIdx.x; j < T; j += step)
    __hip_atomic_store(t.keys + j, GRID_EMPTY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  unsigned long long *r2 = reinterpret_cast<unsigned long long *>(t.rows);
  for (long long j = (long long)blockIdx.x * GM_BLOCK + threadIdx.x; j < T / 2 + 1; j += step)
    __hip_atomic_store(r2 + j, ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// What the three row launches share: the workgroup's keyframe and row, false where it has nothing to do.
struct GmRow {
  int s, k, i, len;
  unsigned g;
};
__device__ __forceinline__ bool gm_row(int MK, int n, const int *__restrict__ state, const int *__restrict__ bank_len,
                                       GmRow &r) {
  r.s = blockIdx.z;
  const int *st = state + (size_t)r.s * GM_WORDS;
  if ((int)blockIdx.y >= st[GM_TODO]) return false;                 // uniform over the workgroup
  r.k = st[GM_BUILT] + (int)blockIdx.y;
  if (r.k < 0 || r.k >= MK) return false;
  r.i = blockIdx.x * GM_BLOCK + threadIdx.x;
  r.len = min(max(bank_len[(size_t)r.s * MK + r.k], 0), n);
  r.g = (unsigned)r.k * (unsigned)n + (unsigned)r.i;
  return true;
}

__global__ __launch_bounds__(GM_BLOCK) void gm_insert_kernel(int S, int MK, int n, int log2T, double voxel,
                                                             const double *__restrict__ X, int frames,
                                                             const float *__restrict__ bank_cloud,
                                                             const int *__restrict__ bank_frame,
                                                             const int *__restrict__ bank_len,
                                                             const int *__restrict__ state,
                                                             unsigned long long *__restrict__ keys,
                                                             unsigned *__restrict__ rows, int *__restrict__ slots) {
  GmRow r;
  if (!gm_row(MK, n, state, bank_len, r) || r.i >= r.len) return;
  const GridTable t = gm_table(keys, rows, r.s, log2T);
  const size_t row = ((size_t)r.s * MK + r.k) * n + r.i;
  float w[3];
  unsigned long long h;
  const bool cand = gm_world(X, frames, S, r.s, bank_frame[(size_t)r.s * MK + r.k], bank_cloud + row * 3, w) &&
                    grid_key(w, voxel, h);
  slots[row] = cand ? grid_insert(t, h, r.g) : -1;
}

// Is this thread's row a winner?  Every lane of the workgroup answers (false past the keyframe's length).
__device__ __forceinline__ bool gm_winner(const GmRow &r, int MK, int n, const GridTable t, const int *__restrict__ slots) {
  if (r.i >= r.len) return false;
  const int slot = slots[((size_t)r.s * MK + r.k) * n + r.i];
  return slot >= 0 && grid_is_winner(t, slot, r.g);
}

__global__ __launch_bounds__(GM_BLOCK) void gm_count_kernel(int MK, int n, int log2T, const int *__restrict__ bank_len,
                                                            const int *__restrict__ state,
                                                            unsigned long long *__restrict__ keys,
                                                            unsigned *__restrict__ rows, const int *__restrict__ slots,
                                                            int *__restrict__ blocks) {
  __shared__ int wave_total[GM_BLOCK / 64];
  GmRow r;
  if (!gm_row(MK, n, state, bank_len, r)) return;
  const bool w = gm_winner(r, MK, n, gm_table(keys, rows, r.s, log2T), slots);
  const int c = __popcll(__ballot(w));
  if ((threadIdx.x & 63) == 0) wave_total[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0)
    blocks[(size_t)r.s * MK * gridDim.x + (size_t)blockIdx.y * gridDim.x + blockIdx.x] =
        (wave_total[0] + wave_total[1]) + (wave_total[2] + wave_total[3]);
}

// One workgroup per stream: blocks[j] = total + the counts of the blocks before j, j < NB todo in (keyframe, block) order;
// total += all of them.  Thread t owns a contiguous chunk; the 256 chunk sums are scanned in LDS.
__global__ __launch_bounds__(GM_BLOCK) void gm_scan_kernel(int MK, int NB, int *__restrict__ state, int *__restrict__ blocks) {
  __shared__ int part[GM_BLOCK];
  const int s = blockIdx.x;
  int *st = state + (size_t)s * GM_WORDS;
  const int todo = st[GM_TODO];
  if (todo <= 0) return;                                            // uniform
  const long long m = (long long)NB * todo;
  int *b = blocks + (size_t)s * MK * NB;
  const long long chunk = (m + GM_BLOCK - 1) / GM_BLOCK;
  const long long j0 = min((long long)threadIdx.x * chunk, m), j1 = min(j0 + chunk, m);
  int sum = 0;
  for (long long j = j0; j < j1; ++j) sum += b[j];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < GM_BLOCK; d <<= 1) {                          // inclusive scan of the chunk sums
    const int v = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  const int total = st[GM_TOTAL];
  int run = total + part[threadIdx.x] - sum;
  for (long long j = j0; j < j1; ++j) {
    const int c = b[j];
    b[j] = run;
    run += c;
  }
  __syncthreads();                                                  // every thread has read the old total
  if (threadIdx.x == 0) st[GM_TOTAL] = total + part[GM_BLOCK - 1];
}

__global__ __launch_bounds__(GM_BLOCK) void gm_write_kernel(int S, int MK, int n, int log2T, int capacity,
                                                            const double *__restrict__ X, int frames,
                                                            const float *__restrict__ bank_cloud,
                                                            const int *__restrict__ bank_frame,
                                                            const int *__restrict__ bank_len,
                                                            const int *__restrict__ state,
                                                            unsigned long long *__restrict__ keys,
                                                            unsigned *__restrict__ rows, const int *__restrict__ slots,
                                                            const int *__restrict__ blocks, float *__restrict__ points,
                                                            int *__restrict__ source) {
  __shared__ int wave_total[GM_BLOCK / 64];
  GmRow r;
  if (!gm_row(MK, n, state, bank_len, r)) return;
  const bool w = gm_winner(r, MK, n, gm_table(keys, rows, r.s, log2T), slots);
  const unsigned long long m = __ballot(w);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) wave_total[wave] = __popcll(m);
  __syncthreads();
  int rank = blocks[(size_t)r.s * MK * gridDim.x + (size_t)blockIdx.y * gridDim.x + blockIdx.x] + mbcnt64(m);
  for (int v = 0; v < wave; ++v) rank += wave_total[v];
  if (!w || rank >= capacity) return;
  const int frame = bank_frame[(size_t)r.s * MK + r.k];
  float o[3];
  gm_world(X, frames, S, r.s, frame, bank_cloud + (((size_t)r.s * MK + r.k) * n + r.i) * 3, o);
  float *pt = points + ((size_t)r.s * capacity + rank) * 3;
  pt[0] = o[0];
  pt[1] = o[1];
  pt[2] = o[2];
  int *src = source + ((size_t)r.s * capacity + rank) * 2;
  src[0] = frame;
  src[1] = r.i;
}

__global__ void gm_end_kernel(int S, int *__restrict__ state) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  int *st = state + (size_t)s * GM_WORDS;
  if (st[GM_RUN] == 0) return;
  st[GM_BUILT] += st[GM_TODO];
  st[GM_DIRTY] = 0;
}

}  // namespace pwclo

using namespace pwclo;

extern "C" long long global_map_bytes(int S, int MK, int n, int capacity) {
  if (!gm_sizes_ok(S, MK, n) || capacity < 1 || (long long)capacity > (long long)MK * n) return 0;
  const long long T = 1ll << gm_table_log2(MK, n), rows = (long long)MK * n;
  return (long long)S * (8 * T + 4 * (T + 2) + 16 * rows + 8ll * MK + 4ll * MK * gm_blocks(n) + 4 * GM_WORDS +
                         20ll * capacity);
}

#define GM_SIZES(what)                                                                                                  \
  PWCLO_REQUIRE(gm_sizes_ok(S, MK, n), what ": S=%d MK=%d n=%d out of range (S <= %d, MK <= %d, MK n <= 2^29)", S, MK, n, \
                GM_MAX_STREAMS, GM_MAX_KEYFRAMES)

extern "C" void global_map_begin_kernel_wrapper(int S, int MK, int n, int stride, int E, int mode, const int *active,
                                                const int *restart, const int *frame_id, const int *lengths, int *state,
                                                int *bank_frame, int *bank_len, int *overflow) {
  GM_SIZES("global_map_begin");
  PWCLO_REQUIRE(stride >= 1 && E >= 1 && E <= MK && (mode == 0 || mode == 1),
                "global_map_begin: stride=%d >= 1, max_new=%d in [1, MK] and mode=%d in {0, 1}", stride, E, mode);
  PWCLO_REQUIRE(state != nullptr && bank_frame != nullptr && bank_len != nullptr && overflow != nullptr &&
                (mode == 1 || frame_id != nullptr),
                "global_map_begin: state, the bank's words, overflow (and frame_id of a streaming call) are required%s", "");
  hipLaunchKernelGGL(gm_begin_kernel, dim3(ceil_div(S, 64)), dim3(64), 0, current_stream(), S, MK, n, stride, E, mode,
                     active, restart, frame_id, lengths, state, bank_frame, bank_len, overflow);
  check_launch("global_map_begin");
}

extern "C" void global_map_push_kernel_wrapper(int S, int MK, int n, const float *cloud, const int *state,
                                               float *bank_cloud) {
  GM_SIZES("global_map_push");
  PWCLO_REQUIRE(cloud != nullptr && state != nullptr && bank_cloud != nullptr,
                "global_map_push: cloud, state and bank_cloud are required%s", "");
  hipLaunchKernelGGL(gm_push_kernel, dim3(gm_blocks(n), S), dim3(GM_BLOCK), 0, current_stream(), MK, n, cloud, state,
                     bank_cloud);
  check_launch("global_map_push");
}

extern "C" void global_map_clear_kernel_wrapper(int S, int MK, int n, const int *state, void *keys, void *rows) {
  GM_SIZES("global_map_clear");
  PWCLO_REQUIRE(state != nullptr && keys != nullptr && rows != nullptr, "global_map_clear: state, keys and rows are required%s",
                "");
  PWCLO_REQUIRE(aligned(keys, 8) && aligned(rows, 8), "global_map_clear: keys and rows must be 8-byte aligned%s", "");
  const int L = gm_table_log2(MK, n);
  const long long want = ((1ll << L) + 4 * GM_BLOCK - 1) / (4 * GM_BLOCK);          // four slots per thread, at most 2048 workgroups
  hipLaunchKernelGGL(gm_clear_kernel, dim3((unsigned)(want < 2048 ? want : 2048), S), dim3(GM_BLOCK), 0, current_stream(), L,
                     state, static_cast<unsigned long long *>(keys), static_cast<unsigned *>(rows));
  check_launch("global_map_clear");
}

#define GM_ROW_ARGS(what)                                                                                                 \
  GM_SIZES(what);                                                                                                         \
  PWCLO_REQUIRE(E >= 1 && E <= MK, what ": max_new=%d outside [1, MK=%d]", E, MK);                                          \
  PWCLO_REQUIRE(bank_len != nullptr && state != nullptr && keys != nullptr && rows != nullptr && slots != nullptr,         \
                what ": the bank's words, state, keys, rows and slots are required%s", "");                                \
  PWCLO_REQUIRE(aligned(keys, 8) && aligned(rows, 8), what ": keys and rows must be 8-byte aligned%s", "")

#define GM_POSE_ARGS(what)                                                                                                \
  PWCLO_REQUIRE(X != nullptr && frames >= 1 && bank_cloud != nullptr && bank_frame != nullptr,                             \
                what ": poses (frames=%d >= 1), bank_cloud and bank_frame are required", frames)

extern "C" void global_map_insert_kernel_wrapper(int S, int MK, int n, int E, double voxel, const double *X, int frames,
                                                 const float *bank_cloud, const int *bank_frame, const int *bank_len,
                                                 const int *state, void *keys, void *rows, int *slots) {
  GM_ROW_ARGS("global_map_insert");
  GM_POSE_ARGS("global_map_insert");
  PWCLO_REQUIRE(grid_voxel_ok(voxel), "global_map_insert: voxel=%g must be finite and > 0", voxel);
  hipLaunchKernelGGL(gm_insert_kernel, dim3(gm_blocks(n), E, S), dim3(GM_BLOCK), 0, current_stream(), S, MK, n,
                     gm_table_log2(MK, n), voxel, X, frames, bank_cloud, bank_frame, bank_len, state,
                     static_cast<unsigned long long *>(keys), static_cast<unsigned *>(rows), slots);
  check_launch("global_map_insert");
}

extern "C" void global_map_count_kernel_wrapper(int S, int MK, int n, int E, const int *bank_len, const int *state,
                                                void *keys, void *rows, const int *slots, int *blocks) {
  GM_ROW_ARGS("global_map_count");
  PWCLO_REQUIRE(blocks != nullptr, "global_map_count: blocks is required%s", "");
  hipLaunchKernelGGL(gm_count_kernel, dim3(gm_blocks(n), E, S), dim3(GM_BLOCK), 0, current_stream(), MK, n,
                     gm_table_log2(MK, n), bank_len, state, static_cast<unsigned long long *>(keys),
                     static_cast<unsigned *>(rows), slots, blocks);
  check_launch("global_map_count");
}

extern "C" void global_map_scan_kernel_wrapper(int S, int MK, int n, int *state, int *blocks) {
  GM_SIZES("global_map_scan");
  PWCLO_REQUIRE(state != nullptr && blocks != nullptr, "global_map_scan: state and blocks are required%s", "");
  hipLaunchKernelGGL(gm_scan_kernel, dim3(S), dim3(GM_BLOCK), 0, current_stream(), MK, gm_blocks(n), state, blocks);
  check_launch("global_map_scan");
}

extern "C" void global_map_write_kernel_wrapper(int S, int MK, int n, int E, int capacity, const double *X, int frames,
                                                const float *bank_cloud, const int *bank_frame, const int *bank_len,
                                                const int *state, void *keys, void *rows, const int *slots,
                                                const int *blocks, float *points, int *source) {
  GM_ROW_ARGS("global_map_write");
  GM_POSE_ARGS("global_map_write");
  PWCLO_REQUIRE(capacity >= 1 && (long long)capacity <= (long long)MK * n, "global_map_write: capacity=%d outside [1, MK n]",
                capacity);
  PWCLO_REQUIRE(blocks != nullptr && points != nullptr && source != nullptr,
                "global_map_write: blocks, points and source are required%s", "");
  hipLaunchKernelGGL(gm_write_kernel, dim3(gm_blocks(n), E, S), dim3(GM_BLOCK), 0, current_stream(), S, MK, n,
                     gm_table_log2(MK, n), capacity, X, frames, bank_cloud, bank_frame, bank_len, state,
                     static_cast<unsigned long long *>(keys), static_cast<unsigned *>(rows), slots, blocks, points, source);
  check_launch("global_map_write");
}

extern "C" void global_map_end_kernel_wrapper(int S, int *state) {
  PWCLO_REQUIRE(S >= 1 && S <= GM_MAX_STREAMS, "global_map_end: S=%d outside [1, %d]", S, GM_MAX_STREAMS);
  PWCLO_REQUIRE(state != nullptr, "global_map_end: state is required%s", "");
  hipLaunchKernelGGL(gm_end_kernel, dim3(ceil_div(S, 64)), dim3(64), 0, current_stream(), S, state);
  check_launch("global_map_end");
}
