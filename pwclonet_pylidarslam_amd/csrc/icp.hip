// Point-to-plane registration of a frame against a sliding local map of the last frames (gfx950).
//
// The reference's ICPFrameToModel (slam/odometry/icp_odometry.py:248-299) refines a learned initial pose by Gauss-Newton on
// point-to-plane residuals against a kd-tree of the last frames, on the host.  Here every map slot keeps its cloud, its
// normals and its neighbour-search structure (knn.hip) in the slot's own frame, built once when the frame arrives; only the
// queries move.  icp.hpp holds the arithmetic; this file holds
//   icp_normals_kernel      normals of a cloud from its own k nearest neighbours
//   icp_queries_kernel      q[s, m, i] = fp32(A[s, m] (T[s]) p[s, i]): the frame's points in every slot's coordinates
//   icp_accumulate_kernel   slot choice, rejection, Huber weights, the sums of the normal equations: one row per workgroup
//   icp_solve_kernel        rows -> 6x6 Cholesky solve -> pose update, freeze flags, diagnostics
//   icp_map_push_kernel     the handover: poses of the live slots re-based on the new frame, the oldest slot replaced
//   icp_begin_kernel        masked registration only: empties the maps of the streams that restart, before the iterations
// One iteration is queries, the existing search (nsample = 1 over S * M clouds), accumulate, solve.  Nothing is sized at run
// time from the data, no kernel uses an atomic, and every sum is added in a fixed order: two runs give the same bits and a
// captured graph serves every frame.
//
// Masked (per-stream) registration: queries, accumulate, solve and map_push take a nullable `active` (S) of device words.
// nullptr is lock step: the kernels compute what they always did.  Otherwise a stream with active[s] == 0 is idle: nothing
// of it changes (its map, its T), its rows of sums are zero and its status is ICP_IDLE.  The word is the same for a whole
// workgroup of queries, accumulate and map_push (blockIdx -> s), so it is a scalar load and the early exit is uniform.
#include <math.h>

#include "common.hpp"
#include "icp.hpp"

extern "C" long long knn_point_build_bytes(int b, int n);

namespace pwclo {

constexpr int ICP_MAX_SLOTS = 64;
constexpr int ICP_SOLVE_THREADS = 1024;     // 32 streams at a time, 32 lanes (one per column of a row) each

// xyz (b, n, 3); idx (b, n, k + 1): the k + 1 nearest of every point in its own cloud, column 0 (the point itself, or a
// duplicate of it) dropped.  normals (b, n, 3) fp32, eig (b, n, 3) fp64 ascending.
__global__ __launch_bounds__(256) void icp_normals_kernel(int n, int k, const float *__restrict__ xyz,
                                                          const int *__restrict__ idx, float *__restrict__ normals,
                                                          double *__restrict__ eig) {
  const int c = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float *xc = xyz + (size_t)c * n * 3;
  const int *ic = idx + ((size_t)c * n + i) * (k + 1);
  const float y[3] = {xc[(size_t)i * 3], xc[(size_t)i * 3 + 1], xc[(size_t)i * 3 + 2]};
  double cov[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int j = 1; j <= k; ++j) {
    const int nb = min(max(ic[j], 0), n - 1);
    const double dx = (double)xc[(size_t)nb * 3] - (double)y[0], dy = (double)xc[(size_t)nb * 3 + 1] - (double)y[1],
                 dz = (double)xc[(size_t)nb * 3 + 2] - (double)y[2];
    cov[0] += dx * dx; cov[1] += dx * dy; cov[2] += dx * dz;
    cov[3] += dy * dy; cov[4] += dy * dz; cov[5] += dz * dz;
  }
  float out[3];
  double val[3];
  icp_normal(cov, y, out, val);
  float *nc = normals + ((size_t)c * n + i) * 3;
  double *ec = eig + ((size_t)c * n + i) * 3;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    nc[a] = out[a];
    ec[a] = val[a];
  }
}

// A (S, M, 4, 4), T (S, 4, 4) or nullptr (the identity), p (S, n, 3) -> q (S, M, n, 3).  The matrix product and the
// matrix-vector product are fp64; one rounding to fp32.  active: (S) or nullptr.
__global__ __launch_bounds__(256) void icp_queries_kernel(int M, int n, const double *__restrict__ A,
                                                          const double *__restrict__ T, const float *__restrict__ p,
                                                          float *__restrict__ q, const int *__restrict__ active) {
  const int sm = blockIdx.y, s = sm / M, i = blockIdx.x * 256 + threadIdx.x;
  if (active != nullptr && active[s] == 0) return;        // idle: the stream's q rows stay as they are
  if (i >= n) return;
  Se3 a;
  if (T != nullptr) {                                     // T first: the branches then share no load, and A and T arrive together
    const Se3 t = se3_load(T + (size_t)s * 16);
    a = se3_mul(se3_load(A + (size_t)sm * 16), t);
  } else {
    a = se3_load(A + (size_t)sm * 16);
  }
  const float *pi = p + ((size_t)s * n + i) * 3;
  const float pt[3] = {pi[0], pi[1], pi[2]};
  double o[3];
  se3_apply(a, pt, o);
  float *qi = q + ((size_t)sm * n + i) * 3;
  qi[0] = (float)o[0]; qi[1] = (float)o[1]; qi[2] = (float)o[2];
}

// p (S, n, 3), q / idx / dist (S, M, n[, 3]) from the search with nsample = 1, map_xyz / map_normals (S, M, n, 3), live
// (S, M), Rm (S, M, 3, 3), T (S, 4, 4) -> partial (S, gridDim.x, ICP_ROW).  A dead slot's idx, dist and map rows are never
// read.  active: (S) or nullptr.
// The slot of a point is the live slot of the smallest dist, the lower slot on a tie.  A NaN dist is never smaller, so one
// in a later slot is passed over; one in the FIRST live slot is taken as the running best, which nothing then beats, and the
// point is rejected (NaN <= max_dist fails) even when a later slot is finite.  The search writes no NaN for finite clouds;
// tests/test_gpu_icp_edges.py pins this rule.  dist = +inf pairs only under max_dist = +inf; an idx outside [0, n) rejects.
__global__ __launch_bounds__(ICP_ACC_THREADS) void icp_accumulate_kernel(
    int M, int n, const float *__restrict__ p, const float *__restrict__ q, const int *__restrict__ idx,
    const float *__restrict__ dist, const float *__restrict__ map_xyz, const float *__restrict__ map_normals,
    const int *__restrict__ live, const double *__restrict__ Rm, const double *__restrict__ T, double sigma, float max_dist,
    double *__restrict__ partial, const int *__restrict__ active) {
  const int s = blockIdx.y, i = blockIdx.x * ICP_ACC_THREADS + threadIdx.x;
  if (active != nullptr && active[s] == 0) {              // idle: a zero row, no gather (the whole workgroup leaves)
    icp_store_zero_row(partial, s);
    return;
  }
  double acc[ICP_TERMS];
#pragma unroll
  for (int e = 0; e < ICP_TERMS; ++e) acc[e] = 0.0;
  if (i < n) {
    int best = -1;
    float bd = 0.0f;
    for (int m = 0; m < M; ++m) {
      if (live[s * M + m] == 0) continue;
      const float d = dist[((size_t)(s * M + m)) * n + i];
      if (best < 0 || d < bd) {                           // strict: on a tie the lower slot stays
        best = m;
        bd = d;
      }
    }
    if (best >= 0 && bd <= max_dist) {                    // NaN fails
      const size_t sm = (size_t)(s * M + best);
      const int j = idx[sm * n + i];
      if (j >= 0 && j < n) {
        const float *yr = map_xyz + (sm * n + j) * 3, *nr = map_normals + (sm * n + j) * 3, *qr = q + (sm * n + i) * 3,
                    *pr = p + ((size_t)s * n + i) * 3;
        const float y[3] = {yr[0], yr[1], yr[2]}, nn[3] = {nr[0], nr[1], nr[2]}, qq[3] = {qr[0], qr[1], qr[2]},
                    pp[3] = {pr[0], pr[1], pr[2]};
        if (nn[0] != 0.0f || nn[1] != 0.0f || nn[2] != 0.0f) {
          double r9[9];
#pragma unroll
          for (int e = 0; e < 9; ++e) r9[e] = Rm[sm * 9 + e];
          icp_add_pair(pp, qq, y, nn, se3_load(T + (size_t)s * 16), r9, sigma, acc);
        }
      }
    }
  }
  icp_reduce_store_row(acc, partial, s);
}

// One workgroup.  32 lanes add the columns of a stream's rows in group order, then one thread per stream solves.
// active: (S) or nullptr; read in iteration 0 only, where it decides the status word a stream starts from.
__global__ __launch_bounds__(ICP_SOLVE_THREADS) void icp_solve_kernel(
    int S, int groups, int it, const double *__restrict__ partial, double damping, double threshold, int min_pairs,
    double *__restrict__ T, int *__restrict__ status, int *__restrict__ iters, int *__restrict__ pairs,
    double *__restrict__ cost, double *__restrict__ sum_out, double *__restrict__ delta_out,
    const int *__restrict__ active) {
  __shared__ double rows[ICP_SOLVE_THREADS / 32][ICP_ROW];
  const int col = threadIdx.x & 31, sl = threadIdx.x >> 5;
  for (int base = 0; base < S; base += ICP_SOLVE_THREADS / 32) {
    __syncthreads();                                       // the previous chunk's rows have been read
    if (base + sl < S) {
      const double *pr = partial + (size_t)(base + sl) * groups * ICP_ROW + col;
      double v = 0.0;
      for (int g = 0; g < groups; ++g) v += pr[(size_t)g * ICP_ROW];
      rows[sl][col] = v;
      sum_out[(size_t)(base + sl) * ICP_ROW + col] = v;
    }
    __syncthreads();
    const int s = base + (int)threadIdx.x;
    if (threadIdx.x < ICP_SOLVE_THREADS / 32 && s < S) {
      double sum[ICP_ROW], delta[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int e = 0; e < ICP_ROW; ++e) sum[e] = rows[threadIdx.x][e];
      int st = it == 0 ? 0 : status[s];
      if (it == 0) iters[s] = 0;
      if (it == 0 && active != nullptr && active[s] == 0) {   // idle: frozen from the start, T is never touched
        st = ICP_IDLE;
        pairs[s] = 0;
        cost[s] = 0.0;
      }
      if (st == 0) {
        const int np = (int)sum[ICP_PAIRS];
        iters[s] = it + 1;
        pairs[s] = np;
        cost[s] = sum[ICP_COST];
        if (np < min_pairs) {
          st = ICP_FEW_PAIRS;
        } else if (!icp_solve6(sum, damping, delta)) {
          st = ICP_BAD_PIVOT;
#pragma unroll
          for (int e = 0; e < 6; ++e) delta[e] = 0.0;
        } else {
          Se3 t = se3_load(T + (size_t)s * 16);
          icp_update_pose(delta, t);
          se3_store_rows(T + (size_t)s * 16, t);                 // row 3 of the caller's matrix stays
          double nd = 0.0;
#pragma unroll
          for (int e = 0; e < 6; ++e) nd += delta[e] * delta[e];
          if (sqrt(nd) < threshold) st = ICP_CONVERGED;
        }
      }
      status[s] = st;
#pragma unroll
      for (int e = 0; e < 6; ++e) delta_out[(size_t)s * 6 + e] = delta[e];
    }
  }
}

// One workgroup per stream.  The staged frame (cloud, normals, the rows and boxes of its search structure, built for S
// clouds) goes into slot cursor[s] of the stream's map (structures built for S * M clouds); the live slots' poses are
// re-based on the new frame; the cursor moves on.  insert (S) or nullptr: the keyframe gate's decision (keyframe.hip,
// DESIGN.md section 23).  nullptr is the ungated push.  A stream with insert[s] == 0 keeps its slots, live flags and cursor:
// nothing is copied and every live slot, the cursor's included, is only re-based.  The word is the same for the whole
// workgroup, so the exit is uniform.  A cursor word outside [0, M) is read as the nearest slot (-1 as 0, M as M - 1), so no
// word can send the copy outside the stream's map; an inserting push then leaves the cursor in range, a push that does not
// insert leaves the word as it found it.
__global__ __launch_bounds__(1024) void icp_map_push_kernel(int M, int n, int S, int nblk, const double *__restrict__ T,
                                                            const float *__restrict__ cloud,
                                                            const float *__restrict__ normals,
                                                            const float4 *__restrict__ stage_ws, float *__restrict__ map_xyz,
                                                            float *__restrict__ map_normals, float4 *__restrict__ map_ws,
                                                            double *__restrict__ A, double *__restrict__ Rm,
                                                            int *__restrict__ live, int *__restrict__ cursor,
                                                            const int *__restrict__ active,
                                                            const int *__restrict__ insert) {
  const int s = blockIdx.x;
  if (active != nullptr && active[s] == 0) return;        // idle: before anything is read
  const bool ins = insert == nullptr || insert[s] != 0;
  const int slot = min(max(cursor[s], 0), M - 1);
  const size_t sm = (size_t)s * M + slot;
  const size_t n3 = (size_t)n * 3, nrow = (size_t)nblk * 64, nbox = (size_t)nblk * 2;
  if (ins) {
    for (size_t j = threadIdx.x; j < n3; j += 1024) {
      map_xyz[sm * n3 + j] = cloud[(size_t)s * n3 + j];
      map_normals[sm * n3 + j] = normals[(size_t)s * n3 + j];
    }
    const float4 *srow = stage_ws + (size_t)s * nrow, *sbox = stage_ws + (size_t)S * nrow + (size_t)s * nbox;
    float4 *drow = map_ws + sm * nrow, *dbox = map_ws + (size_t)S * M * nrow + sm * nbox;
    for (size_t j = threadIdx.x; j < nrow; j += 1024) drow[j] = srow[j];
    for (size_t j = threadIdx.x; j < nbox; j += 1024) dbox[j] = sbox[j];
  }
  const int m = threadIdx.x;
  if (m < M)
    icp_slot_after_push(ins && m == slot, live + s * M + m, A + ((size_t)s * M + m) * 16, T + (size_t)s * 16,
                        Rm + ((size_t)s * M + m) * 9);
  __syncthreads();                                         // everyone has read the cursor
  if (ins && threadIdx.x == 0) cursor[s] = slot + 1 == M ? 0 : slot + 1;
}

// Masked registration, first launch of the body.  One workgroup per stream, one thread per slot: a stream that delivered a
// frame which starts a new sequence (active && (restart || armed)) gets an empty map -- live = 0, cursor = 0, A = R = I --
// and so takes the "no live slot" path of the iterations: it freezes in iteration 0 with ICP_FEW_PAIRS, keeps its initial
// guess and the push fills slot 0.  armed (S) or nullptr: a restart asked for between calls (IcpRefiner.reset(streams)),
// consumed by the stream's next delivered frame.  The slots' clouds and structures stay: nothing reads a dead slot's.
__global__ __launch_bounds__(ICP_MAX_SLOTS) void icp_begin_kernel(int M, const int *__restrict__ active,
                                                                  const int *__restrict__ restart, int *__restrict__ armed,
                                                                  double *__restrict__ A, double *__restrict__ Rm,
                                                                  int *__restrict__ live, int *__restrict__ cursor) {
  const int s = blockIdx.x;
  if (active[s] == 0) return;
  const bool clear = restart[s] != 0 || (armed != nullptr && armed[s] != 0);
  __syncthreads();                                         // everyone has read the armed word
  if (!clear) return;
  const int m = threadIdx.x;
  if (m < M) {
    icp_slot_identity(A + ((size_t)s * M + m) * 16, Rm + ((size_t)s * M + m) * 9);
    live[s * M + m] = 0;
  }
  if (m == 0) {
    cursor[s] = 0;
    if (armed != nullptr) armed[s] = 0;
  }
}

}  // namespace pwclo

using namespace pwclo;

extern "C" void icp_normals_kernel_wrapper(int b, int n, int k, const float *xyz, const int *idx, float *normals,
                                           double *eig) {
  if (b <= 0) return;
  PWCLO_REQUIRE(n >= 2 && (long long)n * 3 < (1ll << 31) && b <= 65535, "icp_normals: b=%d n=%d out of range", b, n);
  PWCLO_REQUIRE(k >= 1 && k <= 63 && k < n, "icp_normals: k=%d outside [1, min(63, n - 1)] for n=%d", k, n);
  PWCLO_REQUIRE((long long)n * (k + 1) < (1ll << 31), "icp_normals: n=%d k=%d neighbour lists too long", n, k);
  PWCLO_REQUIRE(xyz != nullptr && idx != nullptr && normals != nullptr && eig != nullptr && aligned(eig, 8),
                "icp_normals: xyz, idx, normals and eig (8-byte aligned) are required%s", "");
  hipLaunchKernelGGL(icp_normals_kernel, dim3(ceil_div(n, 256), b), dim3(256), 0, current_stream(), n, k, xyz, idx, normals,
                     eig);
  check_launch("icp_normals");
}

// The four entry points below exist twice: the lock-step symbol (active = nullptr) and the masked one share a launcher.
static void icp_queries_launch(const char *what, int S, int M, int n, const double *A, const double *T, const float *p,
                               float *q, const int *active) {
  if (S <= 0) return;
  PWCLO_REQUIRE(M >= 1 && M <= ICP_MAX_SLOTS && n >= 1 && (long long)n * 3 < (1ll << 31) && (long long)S * M <= 65535,
                "%s: S=%d M=%d n=%d out of range (M <= %d, S * M <= 65535)", what, S, M, n, ICP_MAX_SLOTS);
  PWCLO_REQUIRE(A != nullptr && p != nullptr && q != nullptr && aligned(A, 8) && aligned(T, 8),
                "%s: A (8-byte aligned), p and q are required", what);
  hipLaunchKernelGGL(icp_queries_kernel, dim3(ceil_div(n, 256), S * M), dim3(256), 0, current_stream(), M, n, A, T, p, q,
                     active);
  check_launch(what);
}

extern "C" void icp_queries_kernel_wrapper(int S, int M, int n, const double *A, const double *T, const float *p, float *q) {
  icp_queries_launch("icp_queries", S, M, n, A, T, p, q, nullptr);
}

extern "C" void icp_queries_masked_kernel_wrapper(int S, int M, int n, const double *A, const double *T, const float *p,
                                                  float *q, const int *active) {
  PWCLO_REQUIRE(S <= 0 || (active != nullptr && aligned(active, 4)), "icp_queries_masked: active is required%s", "");
  icp_queries_launch("icp_queries_masked", S, M, n, A, T, p, q, active);
}

extern "C" int icp_accumulate_groups(int n) { return n >= 1 ? ceil_div(n, ICP_ACC_THREADS) : 0; }

static void icp_accumulate_launch(const char *what, int S, int M, int n, const float *p, const float *q, const int *idx,
                                  const float *dist, const float *map_xyz, const float *map_normals, const int *live,
                                  const double *R, const double *T, double sigma, float max_dist, double *partial,
                                  const int *active) {
  if (S <= 0) return;
  PWCLO_REQUIRE(M >= 1 && M <= ICP_MAX_SLOTS && n >= 1 && (long long)n * 3 < (1ll << 31) && S <= 65535 &&
                (long long)S * M * n < (1ll << 31),
                "%s: S=%d M=%d n=%d out of range (M <= %d)", what, S, M, n, ICP_MAX_SLOTS);
  PWCLO_REQUIRE(sigma > 0.0 && isfinite(sigma) && max_dist >= 0.0f, "%s: sigma=%g must be > 0, max_dist=%g >= 0", what,
                sigma, (double)max_dist);
  PWCLO_REQUIRE(p != nullptr && q != nullptr && idx != nullptr && dist != nullptr && map_xyz != nullptr &&
                map_normals != nullptr && live != nullptr && R != nullptr && T != nullptr && partial != nullptr,
                "%s: every pointer is required", what);
  PWCLO_REQUIRE(aligned(R, 8) && aligned(T, 8) && aligned(partial, 8),
                "%s: R, T and partial must be 8-byte aligned", what);
  hipLaunchKernelGGL(icp_accumulate_kernel, dim3(icp_accumulate_groups(n), S), dim3(ICP_ACC_THREADS), 0, current_stream(), M,
                     n, p, q, idx, dist, map_xyz, map_normals, live, R, T, sigma, max_dist, partial, active);
  check_launch(what);
}

extern "C" void icp_accumulate_kernel_wrapper(int S, int M, int n, const float *p, const float *q, const int *idx,
                                              const float *dist, const float *map_xyz, const float *map_normals,
                                              const int *live, const double *R, const double *T, double sigma,
                                              float max_dist, double *partial) {
  icp_accumulate_launch("icp_accumulate", S, M, n, p, q, idx, dist, map_xyz, map_normals, live, R, T, sigma, max_dist,
                        partial, nullptr);
}

extern "C" void icp_accumulate_masked_kernel_wrapper(int S, int M, int n, const float *p, const float *q, const int *idx,
                                                     const float *dist, const float *map_xyz, const float *map_normals,
                                                     const int *live, const double *R, const double *T, double sigma,
                                                     float max_dist, double *partial, const int *active) {
  PWCLO_REQUIRE(S <= 0 || (active != nullptr && aligned(active, 4)), "icp_accumulate_masked: active is required%s", "");
  icp_accumulate_launch("icp_accumulate_masked", S, M, n, p, q, idx, dist, map_xyz, map_normals, live, R, T, sigma,
                        max_dist, partial, active);
}

static void icp_solve_launch(const char *what, int S, int groups, int it, const double *partial, double damping,
                             double threshold, int min_pairs, double *T, int *status, int *iters, int *pairs, double *cost,
                             double *sum, double *delta, const int *active) {
  if (S <= 0) return;
  PWCLO_REQUIRE(S <= 65535 && groups >= 1 && it >= 0, "%s: S=%d groups=%d it=%d out of range", what, S, groups, it);
  PWCLO_REQUIRE(damping >= 0.0 && isfinite(damping) && threshold >= 0.0 && min_pairs >= 1,
                "%s: damping=%g and threshold=%g must be >= 0, min_pairs=%d >= 1", what, damping, threshold, min_pairs);
  PWCLO_REQUIRE(partial != nullptr && T != nullptr && status != nullptr && iters != nullptr && pairs != nullptr &&
                cost != nullptr && sum != nullptr && delta != nullptr, "%s: every pointer is required", what);
  PWCLO_REQUIRE(aligned(partial, 8) && aligned(T, 8) && aligned(cost, 8) && aligned(sum, 8) &&
                aligned(delta, 8), "%s: fp64 arrays must be 8-byte aligned", what);
  hipLaunchKernelGGL(icp_solve_kernel, dim3(1), dim3(ICP_SOLVE_THREADS), 0, current_stream(), S, groups, it, partial, damping,
                     threshold, min_pairs, T, status, iters, pairs, cost, sum, delta, active);
  check_launch(what);
}

extern "C" void icp_solve_kernel_wrapper(int S, int groups, int it, const double *partial, double damping, double threshold,
                                         int min_pairs, double *T, int *status, int *iters, int *pairs, double *cost,
                                         double *sum, double *delta) {
  icp_solve_launch("icp_solve", S, groups, it, partial, damping, threshold, min_pairs, T, status, iters, pairs, cost, sum,
                   delta, nullptr);
}

extern "C" void icp_solve_masked_kernel_wrapper(int S, int groups, int it, const double *partial, double damping,
                                                double threshold, int min_pairs, double *T, int *status, int *iters,
                                                int *pairs, double *cost, double *sum, double *delta, const int *active) {
  PWCLO_REQUIRE(S <= 0 || (active != nullptr && aligned(active, 4)), "icp_solve_masked: active is required%s", "");
  icp_solve_launch("icp_solve_masked", S, groups, it, partial, damping, threshold, min_pairs, T, status, iters, pairs, cost,
                   sum, delta, active);
}

static void icp_map_push_launch(const char *what, int S, int M, int n, const double *T, const float *cloud,
                                const float *normals, const void *stage_ws, float *map_xyz, float *map_normals, void *map_ws,
                                double *A, double *R, int *live, int *cursor, const int *active,
                                const int *insert = nullptr) {
  if (S <= 0) return;
  const long long per = knn_point_build_bytes(1, n);       // 0 outside the range the search structure supports
  PWCLO_REQUIRE(per > 0 && M >= 1 && M <= ICP_MAX_SLOTS && (long long)S * M <= 65535,
                "%s: S=%d M=%d n=%d out of range (64 <= n <= 16384, M <= %d, S * M <= 65535)", what, S, M, n,
                ICP_MAX_SLOTS);
  PWCLO_REQUIRE(T != nullptr && cloud != nullptr && normals != nullptr && stage_ws != nullptr && map_xyz != nullptr &&
                map_normals != nullptr && map_ws != nullptr && A != nullptr && R != nullptr && live != nullptr &&
                cursor != nullptr, "%s: every pointer is required", what);
  PWCLO_REQUIRE(aligned(stage_ws, 16) && aligned(map_ws, 16) && aligned(T, 8) && aligned(A, 8) &&
                aligned(R, 8), "%s: structures must be 16-byte, fp64 arrays 8-byte aligned", what);
  const int nblk = (int)(per / (64 * 16 + 32));
  hipLaunchKernelGGL(icp_map_push_kernel, dim3(S), dim3(1024), 0, current_stream(), M, n, S, nblk, T, cloud, normals,
                     static_cast<const float4 *>(stage_ws), map_xyz, map_normals, static_cast<float4 *>(map_ws), A, R, live,
                     cursor, active, insert);
  check_launch(what);
}

extern "C" void icp_map_push_kernel_wrapper(int S, int M, int n, const double *T, const float *cloud, const float *normals,
                                            const void *stage_ws, float *map_xyz, float *map_normals, void *map_ws, double *A,
                                            double *R, int *live, int *cursor) {
  icp_map_push_launch("icp_map_push", S, M, n, T, cloud, normals, stage_ws, map_xyz, map_normals, map_ws, A, R, live, cursor,
                      nullptr);
}

extern "C" void icp_map_push_masked_kernel_wrapper(int S, int M, int n, const double *T, const float *cloud,
                                                   const float *normals, const void *stage_ws, float *map_xyz,
                                                   float *map_normals, void *map_ws, double *A, double *R, int *live,
                                                   int *cursor, const int *active) {
  PWCLO_REQUIRE(S <= 0 || (active != nullptr && aligned(active, 4)), "icp_map_push_masked: active is required%s", "");
  icp_map_push_launch("icp_map_push_masked", S, M, n, T, cloud, normals, stage_ws, map_xyz, map_normals, map_ws, A, R, live,
                      cursor, active);
}

// The push behind the keyframe gate: icp_map_push_masked's launch with the gate's decision word.
// active: (S) or nullptr, as there.
extern "C" void keyframe_icp_push_kernel_wrapper(int S, int M, int n, const double *T, const float *cloud,
                                                 const float *normals, const void *stage_ws, float *map_xyz,
                                                 float *map_normals, void *map_ws, double *A, double *R, int *live,
                                                 int *cursor, const int *active, const int *insert) {
  PWCLO_REQUIRE(S <= 0 || (insert != nullptr && aligned(insert, 4) && aligned(active, 4)),
                "keyframe_icp_push: insert is required, and insert and active must be 4-byte aligned%s", "");
  icp_map_push_launch("keyframe_icp_push", S, M, n, T, cloud, normals, stage_ws, map_xyz, map_normals, map_ws, A, R, live,
                      cursor, active, insert);
}

extern "C" void icp_begin_kernel_wrapper(int S, int M, const int *active, const int *restart, int *armed, double *A,
                                         double *R, int *live, int *cursor) {
  if (S <= 0) return;
  PWCLO_REQUIRE(M >= 1 && M <= ICP_MAX_SLOTS && (long long)S * M <= 65535,
                "icp_begin: S=%d M=%d out of range (M <= %d, S * M <= 65535)", S, M, ICP_MAX_SLOTS);
  PWCLO_REQUIRE(active != nullptr && restart != nullptr && A != nullptr && R != nullptr && live != nullptr &&
                cursor != nullptr, "icp_begin: every pointer but armed is required%s", "");
  PWCLO_REQUIRE(aligned(A, 8) && aligned(R, 8) && aligned(active, 4) && aligned(restart, 4) &&
                aligned(armed, 4), "icp_begin: fp64 arrays must be 8-byte, mask words 4-byte aligned%s", "");
  hipLaunchKernelGGL(icp_begin_kernel, dim3(S), dim3(ICP_MAX_SLOTS), 0, current_stream(), M, active, restart, armed, A, R,
                     live, cursor);
  check_launch("icp_begin");
}
