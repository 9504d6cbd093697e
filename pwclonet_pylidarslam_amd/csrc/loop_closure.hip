// Loop detection on the device: Scan Context descriptors (Kim & Kim, IROS 2018), an exhaustive
// circular-correlation search over every stored place, and the bookkeeping that hands a verified closure to the pose graph.
// One detection = build, score, select, fetch, (two registrations of registration.IcpRefiner), accept, insert.  Every sum
// has a fixed order; the only atomic is the LDS max of the descriptor, which is order-free; there is no spinning and no loop
// whose bound is read from memory.
#include "loop_closure.hpp"

namespace pwclo {

// ---- build: one workgroup per stream ---------------------------------------------------------------------------------------

struct LcBuild {
  int S, n, NR, NS, up_neg_y;
  float z_offset;
  const float *cloud;               // (S, n, 3)
  const int *lengths;               // (S) or null: rows [0, min(max(lengths[s], 0), n)) count
  const float *ring_b;              // (NR): b_1 .. b_NR
  const float *sector_d;            // (NS, 2)
  float *D, *Dn;                    // (S, NR, NS)
  unsigned long long *mask;         // (S)
  const int *active, *restart;      // (S) or null
  int *count, *nlog, *epoch;        // (S) or null: the detector's words, emptied where active and restart
};

__global__ __launch_bounds__(LC_BUILD_THREADS) void lc_build_kernel(LcBuild a) {
  extern __shared__ unsigned lc_cells[];            // NR * NS bit patterns of positive floats (0: empty)
  __shared__ float tab_b[LC_MAX_RINGS];
  __shared__ float tab_d[2 * LC_MAX_SECTORS];
  const int s = blockIdx.x, tid = threadIdx.x;
  if (a.active != nullptr && a.active[s] == 0) return;          // an idle stream keeps every word
  if (tid == 0 && a.count != nullptr && a.restart != nullptr && a.restart[s] != 0) {
    a.count[s] = 0;
    a.nlog[s] = 0;
    a.epoch[s] += 1;
  }
  const int NR = a.NR, NS = a.NS, cells = NR * NS;
  for (int i = tid; i < cells; i += LC_BUILD_THREADS) lc_cells[i] = 0u;
  if (tid < NR) tab_b[tid] = a.ring_b[tid];
  if (tid < 2 * NS) tab_d[tid] = a.sector_d[tid];
  __syncthreads();
  int len = a.n;
  if (a.lengths != nullptr) len = min(max(a.lengths[s], 0), a.n);
  const float *p = a.cloud + (size_t)s * a.n * 3;
  const float b_last = tab_b[NR - 1];
  for (int i = tid; i < a.n; i += LC_BUILD_THREADS) {
    if (i >= len) continue;
    const float c0 = p[3 * i], c1 = p[3 * i + 1], c2 = p[3 * i + 2];
    if (!(lc_finite(c0) && lc_finite(c1) && lc_finite(c2))) continue;
    const float x = a.up_neg_y ? c2 : c0, y = a.up_neg_y ? -c0 : c1, z = a.up_neg_y ? -c1 : c2;
    const float r2 = x * x + y * y;
    const float h = z + a.z_offset;
    if (r2 >= b_last || r2 == 0.f || !(h > 0.f)) continue;
    const int sec = lc_sector(tab_d, NS, x, y);
    if (sec < 0) continue;
    atomicMax(&lc_cells[lc_ring(tab_b, NR, r2) * NS + sec], __float_as_uint(h));
  }
  __syncthreads();
  float *D = a.D + (size_t)s * cells, *Dn = a.Dn + (size_t)s * cells;
  if (tid < 64) {                                   // wave 0: one column per lane
    float norm = 0.f;
    if (tid < NS) {
      float sum = 0.f;
      for (int r = 0; r < NR; ++r) {
        const float v = __uint_as_float(lc_cells[r * NS + tid]);
        sum = sum + v * v;
      }
      norm = sqrtf(sum);
      for (int r = 0; r < NR; ++r) {
        const float v = __uint_as_float(lc_cells[r * NS + tid]);
        D[r * NS + tid] = v;
        Dn[r * NS + tid] = norm > 0.f ? v / norm : 0.f;
      }
    }
    const unsigned long long m = __ballot(norm > 0.f);
    if (tid == 0) a.mask[s] = m;
  }
}

// ---- score: one wave per entry, lane = shift -------------------------------------------------------------------------------

struct LcScore {
  int S, NR, NS, MK, min_id_distance, traj_frames;
  double max_distance2;             // the gate compares squared distances; traj null: no gate
  const float *Qn;                  // (S, NR, NS)
  const unsigned long long *qmask;  // (S)
  const float *db_desc;             // (S, MK, NS, NR): an entry's columns, each contiguous
  const unsigned long long *db_mask;// (S, MK)
  const int *db_frame;              // (S, MK)
  const int *count, *active, *frame_id;
  const double *traj;               // (traj_frames, S, 4, 4) or null
  float *scores;                    // (S, MK)
  int *shifts;                      // (S, MK)
};

__global__ __launch_bounds__(LC_SCORE_WAVES * 64) void lc_score_kernel(LcScore a) {
  extern __shared__ float lc_q2[];                  // [NR][2 NS]: the query doubled along the sectors
  const int s = blockIdx.y, tid = threadIdx.x, NR = a.NR, NS = a.NS, W = 2 * NS;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int e = blockIdx.x * LC_SCORE_WAVES + wave;
  const bool act = a.active == nullptr || a.active[s] != 0;
  const int cnt = a.count[s], f = a.frame_id[s];
  if (act && blockIdx.x * LC_SCORE_WAVES < cnt) {   // a workgroup beyond the database stages nothing
    const float *Q = a.Qn + (size_t)s * NR * NS;
    for (int i = tid; i < NR * W; i += LC_SCORE_WAVES * 64) {
      const int r = i / W, c = i - r * W;
      lc_q2[i] = Q[r * NS + (c >= NS ? c - NS : c)];
    }
  }
  __syncthreads();
  if (e >= a.MK) return;
  const size_t at = (size_t)s * a.MK + e;
  bool ok = act && e < cnt;
  int fe = 0;
  if (ok) {
    fe = a.db_frame[at];
    ok = fe + a.min_id_distance <= f;
  }
  if (ok && a.traj != nullptr) {
    ok = f >= 0 && f < a.traj_frames && fe >= 0 && fe < a.traj_frames;
    if (ok) {
      const double *te = a.traj + ((size_t)fe * a.S + s) * 16, *tq = a.traj + ((size_t)f * a.S + s) * 16;
      const double dx = te[3] - tq[3], dy = te[7] - tq[7], dz = te[11] - tq[11];
      const double d2 = (dx * dx + dy * dy) + dz * dz;
      ok = d2 < a.max_distance2;
    }
  }
  if (!ok) {                                        // wave-uniform: not stored, too recent or too far
    if (lane == 0) {
      a.scores[at] = __builtin_inff();
      a.shifts[at] = 0;
    }
    return;
  }
  const int sh = lane < NS ? lane : 0;
  const float *__restrict__ E = a.db_desc + at * (size_t)(NS * NR);      // wave-uniform: scalar loads
  const float *q = lc_q2 + sh;
  float acc = 0.f;
  for (int j = 0; j < NS; ++j) {
    const float *col = E + j * NR;
#pragma unroll 4
    for (int r = 0; r < NR; ++r) acc = acc + q[r * W + j] * col[r];
  }
  const int v = __popcll(lc_rotate(a.qmask[s], NS, sh) & a.db_mask[at]);
  float d = (lane < NS && v > 0) ? 1.f - acc / (float)v : __builtin_inff();
  int best = lane;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float od = __shfl_xor(d, off, 64);
    const int ob = __shfl_xor(best, off, 64);
    if (od < d || (od == d && ob < best)) {
      d = od;
      best = ob;
    }
  }
  if (lane == 0) {
    a.scores[at] = d;
    a.shifts[at] = best;
  }
}

// ---- select: one workgroup per stream ----------------------------------------------------------------------------------------

struct LcSelect {
  int S, NS, MK, stride;
  float threshold;
  const float *scores;
  const int *shifts, *db_frame, *count, *active, *frame_id;
  const double *T0_table;           // (NS, 4, 4): the start pose of every shift
  int *match;                       // (S, 4): found, entry, frame_i, shift
  float *match_score;               // (S)
  int *found;                       // (S)
  double *T0;                       // (S, 4, 4)
  int *slot;                        // (S): where insert writes this call's frame, -1: nowhere
  int *overflow;                    // (1)
};

__global__ __launch_bounds__(LC_SELECT_THREADS) void lc_select_kernel(LcSelect a) {
  __shared__ float red_d[LC_SELECT_THREADS];
  __shared__ int red_e[LC_SELECT_THREADS];
  const int s = blockIdx.x, tid = threadIdx.x;
  const bool act = a.active == nullptr || a.active[s] != 0;
  float d = __builtin_inff();
  int e = a.MK;
  if (act) {
    const float *sc = a.scores + (size_t)s * a.MK;
    for (int i = tid; i < a.MK; i += LC_SELECT_THREADS) {         // ascending per thread: strict < keeps the lowest entry
      const float v = sc[i];
      if (v < d) {
        d = v;
        e = i;
      }
    }
  }
  red_d[tid] = d;
  red_e[tid] = e;
  __syncthreads();
  for (int half = LC_SELECT_THREADS / 2; half >= 1; half >>= 1) {
    if (tid < half) {
      const float od = red_d[tid + half];
      const int oe = red_e[tid + half];
      if (od < red_d[tid] || (od == red_d[tid] && oe < red_e[tid])) {
        red_d[tid] = od;
        red_e[tid] = oe;
      }
    }
    __syncthreads();
  }
  d = red_d[0];
  e = red_e[0];
  const bool any = e < a.MK;                        // a finite score exists
  const bool hit = any && d < a.threshold;
  const int shift = any ? a.shifts[(size_t)s * a.MK + e] : 0;
  if (tid == 0) {
    int *m = a.match + (size_t)s * LC_MATCH;
    m[0] = hit ? 1 : 0;
    m[1] = any ? e : -1;
    m[2] = any ? a.db_frame[(size_t)s * a.MK + e] : -1;
    m[3] = shift;
    a.match_score[s] = d;
    a.found[s] = hit ? 1 : 0;
    int where = -1;
    if (act) {
      const int f = a.frame_id[s], cnt = a.count[s];
      if (f >= 0 && f % a.stride == 0) {
        if (cnt < a.MK) where = cnt;
        else *a.overflow = 1;
      }
    }
    a.slot[s] = where;
  }
  if (tid < 16) {
    const int r = tid >> 2, c = tid & 3;
    a.T0[(size_t)s * 16 + tid] = hit ? a.T0_table[(size_t)shift * 16 + tid] : (r == c ? 1.0 : 0.0);
  }
}

// ---- fetch, insert: grid (LC_COPY_BLOCKS, S) ---------------------------------------------------------------------------------

__global__ __launch_bounds__(LC_COPY_THREADS) void lc_fetch_kernel(int n, int MK, const int *__restrict__ found,
                                                                   const int *__restrict__ match,
                                                                   const float *__restrict__ db_cloud,
                                                                   float *__restrict__ staging) {
  const int s = blockIdx.y;
  if (found[s] == 0) return;
  const int e = match[(size_t)s * LC_MATCH + 1];
  if (e < 0 || e >= MK) return;
  const float *src = db_cloud + ((size_t)s * MK + e) * n * 3;
  float *dst = staging + (size_t)s * n * 3;
  for (int i = blockIdx.x * LC_COPY_THREADS + threadIdx.x; i < n * 3; i += LC_COPY_BLOCKS * LC_COPY_THREADS) dst[i] = src[i];
}

struct LcInsert {
  int S, n, NR, NS, MK;
  const int *slot, *frame_id;
  const float *Qn;
  const unsigned long long *qmask;
  const float *cloud;               // (S, n, 3) or null (no verification: no clouds are kept)
  float *db_desc;
  unsigned long long *db_mask;
  int *db_frame;
  float *db_cloud;
  int *count;
};

__global__ __launch_bounds__(LC_COPY_THREADS) void lc_insert_kernel(LcInsert a) {
  const int s = blockIdx.y;
  const int e = a.slot[s];                          // select's decision: no block of this launch reads count
  if (e < 0 || e >= a.MK) return;
  const int first = blockIdx.x * LC_COPY_THREADS + threadIdx.x, step = LC_COPY_BLOCKS * LC_COPY_THREADS;
  const int cells = a.NR * a.NS;
  const size_t at = (size_t)s * a.MK + e;
  const float *Q = a.Qn + (size_t)s * cells;
  float *E = a.db_desc + at * cells;
  for (int i = first; i < cells; i += step) {       // transposed: E[j][r] = Qn[r][j]
    const int j = i / a.NR, r = i - j * a.NR;
    E[i] = Q[r * a.NS + j];
  }
  if (a.cloud != nullptr) {
    const float *src = a.cloud + (size_t)s * a.n * 3;
    float *dst = a.db_cloud + at * a.n * 3;
    for (int i = first; i < a.n * 3; i += step) dst[i] = src[i];
  }
  if (first == 0) {
    a.db_mask[at] = a.qmask[s];
    a.db_frame[at] = a.frame_id[s];
    a.count[s] = e + 1;
  }
}

// ---- accept: one thread per stream -------------------------------------------------------------------------------------------

struct LcAccept {
  int S, n, ML;
  double min_fitness, max_mean_cost;
  const int *found, *match;
  const float *match_score;
  const int *frame_id;
  const double *T;                  // (S, 4, 4): the refiner's pose, or T0 without verification
  const int *status, *pairs;        // the refiner's words, or null: every match is accepted
  const double *cost;
  int *log_i;                       // (S, ML, 4): i, j, shift, pairs
  double *log_T;                    // (S, ML, 4, 4)
  double *log_c;                    // (S, ML, 2): score, cost
  int *nlog;                        // (S)
  int *log_overflow;                // (1)
  int *accepted;                    // (S): this call's decision
};

__global__ __launch_bounds__(1024) void lc_accept_kernel(LcAccept a) {
  const int s = threadIdx.x;
  if (s >= a.S) return;
  a.accepted[s] = 0;
  if (a.found[s] == 0) return;
  int pairs = 0;
  double cost = 0.0;
  if (a.status != nullptr) {
    pairs = a.pairs[s];
    cost = a.cost[s];
    if ((a.status[s] & (LC_ICP_FEW_PAIRS | LC_ICP_BAD_PIVOT)) != 0) return;
    if (!((double)pairs >= a.min_fitness * (double)a.n)) return;
    if (!(cost / (double)pairs <= a.max_mean_cost)) return;
  }
  const int l = a.nlog[s];
  if (l >= a.ML) {
    *a.log_overflow = 1;
    return;
  }
  const size_t at = (size_t)s * a.ML + l;
  const int *m = a.match + (size_t)s * LC_MATCH;
  int *li = a.log_i + at * LC_LOG_I;
  li[0] = m[2];
  li[1] = a.frame_id[s];
  li[2] = m[3];
  li[3] = pairs;
  for (int k = 0; k < 16; ++k) a.log_T[at * 16 + k] = a.T[(size_t)s * 16 + k];
  a.log_c[at * LC_LOG_C] = (double)a.match_score[s];
  a.log_c[at * LC_LOG_C + 1] = cost;
  a.nlog[s] = l + 1;
  a.accepted[s] = 1;
}

}  // namespace pwclo

using namespace pwclo;

static bool lc_shape(const char *what, int S, int NR, int NS) {
  if (!(S >= 1 && S <= LC_MAX_STREAMS)) {
    set_error(PWCLO_EINVAL, "%s: S=%d streams outside [1, %d]", what, S, LC_MAX_STREAMS);
    return false;
  }
  if (!(NR >= 1 && NR <= LC_MAX_RINGS) || !(NS >= LC_MIN_SECTORS && NS <= LC_MAX_SECTORS)) {
    set_error(PWCLO_EINVAL, "%s: rings=%d outside [1, %d] or sectors=%d outside [%d, %d]", what, NR, LC_MAX_RINGS, NS,
              LC_MIN_SECTORS, LC_MAX_SECTORS);
    return false;
  }
  return true;
}

extern "C" void scan_context_build_kernel_wrapper(int S, int n, int NR, int NS, int up_neg_y, float z_offset,
                                                  const float *cloud, const int *lengths, const float *ring_b,
                                                  const float *sector_d, float *D, float *Dn, void *mask, const int *active,
                                                  const int *restart, int *count, int *nlog, int *epoch) {
  if (!lc_shape("scan_context_build", S, NR, NS)) return;
  PWCLO_REQUIRE(n >= 1 && n <= (1 << 24), "scan_context_build: n=%d points outside [1, 2^24]", n);
  PWCLO_REQUIRE(cloud && ring_b && sector_d && D && Dn && mask, "scan_context_build: a null argument");
  PWCLO_REQUIRE((count != nullptr) == (nlog != nullptr) && (count != nullptr) == (epoch != nullptr),
                "scan_context_build: count, nlog and epoch come together");
  LcBuild a{S, n, NR, NS, up_neg_y != 0, z_offset, cloud, lengths, ring_b, sector_d, D, Dn, (unsigned long long *)mask,
            active, restart, count, nlog, epoch};
  hipLaunchKernelGGL(lc_build_kernel, dim3(S), dim3(LC_BUILD_THREADS), NR * NS * sizeof(unsigned), current_stream(), a);
  check_launch("scan_context_build");
}

extern "C" void loop_score_kernel_wrapper(int S, int NR, int NS, int MK, const float *Qn, const void *qmask,
                                          const float *db_desc, const void *db_mask, const int *db_frame, const int *count,
                                          const int *active, const int *frame_id, int min_id_distance, const double *traj,
                                          int traj_frames, double max_distance, float *scores, int *shifts) {
  if (!lc_shape("loop_score", S, NR, NS)) return;
  PWCLO_REQUIRE(MK >= 1 && MK <= (1 << 20), "loop_score: max_keyframes=%d outside [1, 2^20]", MK);
  PWCLO_REQUIRE(min_id_distance >= 0, "loop_score: min_id_distance=%d must be >= 0", min_id_distance);
  PWCLO_REQUIRE(Qn && qmask && db_desc && db_mask && db_frame && count && frame_id && scores && shifts,
                "loop_score: a null argument");
  PWCLO_REQUIRE(traj == nullptr || (traj_frames >= 1 && max_distance > 0.0),
                "loop_score: a trajectory needs traj_frames=%d >= 1 and max_distance=%g > 0", traj_frames, max_distance);
  LcScore a{S, NR, NS, MK, min_id_distance, traj_frames, max_distance * max_distance, Qn,
            (const unsigned long long *)qmask, db_desc, (const unsigned long long *)db_mask, db_frame, count, active,
            frame_id, traj, scores, shifts};
  hipLaunchKernelGGL(lc_score_kernel, dim3(ceil_div(MK, LC_SCORE_WAVES), S), dim3(LC_SCORE_WAVES * 64),
                     NR * 2 * NS * sizeof(float), current_stream(), a);
  check_launch("loop_score");
}

extern "C" void loop_select_kernel_wrapper(int S, int NS, int MK, int stride, float threshold, const float *scores,
                                           const int *shifts, const int *db_frame, const int *count, const int *active,
                                           const int *frame_id, const double *T0_table, int *match, float *match_score,
                                           int *found, double *T0, int *slot, int *overflow) {
  if (!lc_shape("loop_select", S, 1, NS)) return;
  PWCLO_REQUIRE(MK >= 1 && MK <= (1 << 20), "loop_select: max_keyframes=%d outside [1, 2^20]", MK);
  PWCLO_REQUIRE(stride >= 1, "loop_select: stride=%d must be >= 1", stride);
  PWCLO_REQUIRE(scores && shifts && db_frame && count && frame_id && T0_table && match && match_score && found && T0 &&
                    slot && overflow,
                "loop_select: a null argument");
  LcSelect a{S, NS, MK, stride, threshold, scores, shifts, db_frame, count, active, frame_id, T0_table, match, match_score,
             found, T0, slot, overflow};
  hipLaunchKernelGGL(lc_select_kernel, dim3(S), dim3(LC_SELECT_THREADS), 0, current_stream(), a);
  check_launch("loop_select");
}

extern "C" void loop_fetch_kernel_wrapper(int S, int n, int MK, const int *found, const int *match, const float *db_cloud,
                                          float *staging) {
  PWCLO_REQUIRE(S >= 1 && S <= LC_MAX_STREAMS, "loop_fetch: S=%d streams outside [1, %d]", S, LC_MAX_STREAMS);
  PWCLO_REQUIRE(n >= 1 && n <= (1 << 24) && MK >= 1 && MK <= (1 << 20), "loop_fetch: n=%d or max_keyframes=%d out of range",
                n, MK);
  PWCLO_REQUIRE(found && match && db_cloud && staging, "loop_fetch: a null argument");
  hipLaunchKernelGGL(lc_fetch_kernel, dim3(LC_COPY_BLOCKS, S), dim3(LC_COPY_THREADS), 0, current_stream(), n, MK, found,
                     match, db_cloud, staging);
  check_launch("loop_fetch");
}

extern "C" void loop_accept_kernel_wrapper(int S, int n, int ML, const int *found, const int *match,
                                           const float *match_score, const int *frame_id, const double *T, const int *status,
                                           const int *pairs, const double *cost, double min_fitness, double max_mean_cost,
                                           int *log_i, double *log_T, double *log_c, int *nlog, int *log_overflow,
                                           int *accepted) {
  PWCLO_REQUIRE(S >= 1 && S <= LC_MAX_STREAMS, "loop_accept: S=%d streams outside [1, %d]", S, LC_MAX_STREAMS);
  PWCLO_REQUIRE(n >= 1 && ML >= 1, "loop_accept: n=%d and max_loops=%d must be >= 1", n, ML);
  PWCLO_REQUIRE(found && match && match_score && frame_id && T && log_i && log_T && log_c && nlog && log_overflow && accepted,
                "loop_accept: a null argument");
  PWCLO_REQUIRE((status != nullptr) == (pairs != nullptr) && (status != nullptr) == (cost != nullptr),
                "loop_accept: status, pairs and cost come together");
  LcAccept a{S, n, ML, min_fitness, max_mean_cost, found, match, match_score, frame_id, T, status, pairs, cost, log_i, log_T,
             log_c, nlog, log_overflow, accepted};
  hipLaunchKernelGGL(lc_accept_kernel, dim3(1), dim3(ceil_div(S, 64) * 64), 0, current_stream(), a);
  check_launch("loop_accept");
}

extern "C" void loop_insert_kernel_wrapper(int S, int n, int NR, int NS, int MK, const int *slot, const int *frame_id,
                                           const float *Qn, const void *qmask, const float *cloud, float *db_desc,
                                           void *db_mask, int *db_frame, float *db_cloud, int *count) {
  if (!lc_shape("loop_insert", S, NR, NS)) return;
  PWCLO_REQUIRE(n >= 1 && n <= (1 << 24) && MK >= 1 && MK <= (1 << 20), "loop_insert: n=%d or max_keyframes=%d out of range",
                n, MK);
  PWCLO_REQUIRE(slot && frame_id && Qn && qmask && db_desc && db_mask && db_frame && count, "loop_insert: a null argument");
  PWCLO_REQUIRE((cloud != nullptr) == (db_cloud != nullptr), "loop_insert: cloud and db_cloud come together");
  LcInsert a{S, n, NR, NS, MK, slot, frame_id, Qn, (const unsigned long long *)qmask, cloud, db_desc,
             (unsigned long long *)db_mask, db_frame, db_cloud, count};
  hipLaunchKernelGGL(lc_insert_kernel, dim3(LC_COPY_BLOCKS, S), dim3(LC_COPY_THREADS), 0, current_stream(), a);
  check_launch("loop_insert");
}
