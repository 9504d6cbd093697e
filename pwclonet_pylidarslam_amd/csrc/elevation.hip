// Translation search of the loop detector: between Scan Context's select and the verifying
// registration, the matched place's stored cloud and the query under Y yaw candidates are imaged as G x G grids of 8-bit
// height levels, every planar offset (a, b) in [-W, W]^2 of every candidate is scored by an integer agreement sum, and the
// best seeds the refiner.  image, score, choose.  Every sum is an integer one, so no order matters; the only atomics are the
// LDS max of a cell and the LDS counter that hands out list slots (the list's order is free); there is no spinning.
#include "elevation.hpp"

namespace pwclo {

// ---- image: grid (1 + Y, S); block 0 images E at the identity, block 1 + k the query under candidate k ----------------------

struct ElImage {
  int S, n, NS, G, Y, up_neg_y;
  float z_offset, c, zs;
  const float *cloud;               // (S, n, 3): the query
  const float *staging;             // (S, n, 3): the matched place's stored cloud, imaged whole
  const int *lengths;               // (S) or null: rows [0, min(max(lengths[s], 0), n)) of the query count
  const int *found, *match;         // select's words: found (S), match (S, 4) with the shift in word 3
  const float *rot;                 // (NS Y, 2): cos, sin of theta, row shift * Y + k
  unsigned char *img;               // (S, 1 + Y, G, G): the highest level of every cell, 0: empty
  int *occ;                         // (S, 1 + Y): the non-empty cells
  int *list;                        // (S, Y, G G): i | j << 8 | q << 16 of the non-empty cells of Q_k, in any order
};

__global__ __launch_bounds__(EL_IMAGE_THREADS) void el_image_kernel(ElImage a) {
  extern __shared__ unsigned el_cells[];            // G * G maxima, then the list counter
  const int s = blockIdx.y, v = blockIdx.x, tid = threadIdx.x;
  if (a.found[s] == 0) return;
  const int G = a.G, cells = G * G, lane = tid & 63;
  const int shift = a.match[(size_t)s * LC_MATCH + 3];
  const bool sane = shift >= 0 && shift < a.NS;     // select wrote it; a shift outside the table images nothing
  for (int i = tid; i <= cells; i += EL_IMAGE_THREADS) el_cells[i] = 0u;
  __syncthreads();
  float cs = 1.f, sn = 0.f;
  int len = a.n;
  const float *p = a.staging + (size_t)s * a.n * 3;
  if (v > 0) {
    p = a.cloud + (size_t)s * a.n * 3;
    if (a.lengths != nullptr) len = min(max(a.lengths[s], 0), a.n);
    if (sane) {
      const float *r = a.rot + ((size_t)shift * a.Y + (v - 1)) * 2;
      cs = r[0];
      sn = r[1];
    }
  }
  if (!sane) len = 0;
  for (int r = tid; r < len; r += EL_IMAGE_THREADS) {
    const float c0 = p[3 * r], c1 = p[3 * r + 1], c2 = p[3 * r + 2];
    if (!(lc_finite(c0) && lc_finite(c1) && lc_finite(c2))) continue;
    const float x = a.up_neg_y ? c2 : c0, y = a.up_neg_y ? -c0 : c1, z = a.up_neg_y ? -c1 : c2;
    int i, j, q;
    if (!el_cell(x, y, z, cs, sn, a.c, a.zs, a.z_offset, G, i, j, q)) continue;
    atomicMax(&el_cells[i * G + j], (unsigned)q);
  }
  __syncthreads();
  unsigned char *img = a.img + ((size_t)s * (1 + a.Y) + v) * cells;
  int *list = v > 0 ? a.list + ((size_t)s * a.Y + (v - 1)) * cells : nullptr;
  for (int base = 0; base < cells; base += EL_IMAGE_THREADS) {      // block-uniform trip count: the ballot sees whole waves
    const int at = base + tid;
    const unsigned q = at < cells ? el_cells[at] : 0u;
    if (at < cells) img[at] = (unsigned char)q;
    const unsigned long long full = __ballot(q != 0u);
    int first = 0;
    if (lane == 0 && full != 0ull) first = (int)atomicAdd(&el_cells[cells], (unsigned)__popcll(full));
    first = __shfl(first, 0, 64);
    if (q != 0u && list != nullptr) {
      const int slot = first + __popcll(full & ((1ull << lane) - 1ull));
      const int i = at / G, j = at - i * G;
      if (slot < cells) list[slot] = i | (j << 8) | ((int)q << 16);
    }
  }
  __syncthreads();
  if (tid == 0) a.occ[(size_t)s * (1 + a.Y) + v] = (int)el_cells[cells];
}

// ---- score: grid (blocks, Y, S), one wave per 64 consecutive candidates of one (stream, k), lane = candidate -----------------

struct ElScore {
  int S, G, Y, W, L;
  const int *found;
  const unsigned char *img;         // (S, 1 + Y, G, G): image 0 is E
  const int *occ;                   // (S, 1 + Y)
  const int *list;                  // (S, Y, G G)
  int *A;                           // (S, Y, 2W+1, 2W+1)
};

__global__ __launch_bounds__(EL_SCORE_WAVES * 64) void el_score_kernel(ElScore a) {
  extern __shared__ unsigned char el_E[];           // (G + 2W)^2: E inside a zero border of W cells, so no lane tests a bound
  const int s = blockIdx.z, k = blockIdx.y, tid = threadIdx.x;
  if (a.found[s] == 0) return;
  const int G = a.G, W = a.W, P = G + 2 * W, side = 2 * W + 1, C = side * side, cells = G * G;
  const unsigned char *E = a.img + (size_t)s * (1 + a.Y) * cells;
  for (int at = tid; at < P * P; at += EL_SCORE_WAVES * 64) {
    const int r = at / P, c = at - r * P, i = r - W, j = c - W;
    el_E[at] = (i >= 0 && i < G && j >= 0 && j < G) ? E[i * G + j] : (unsigned char)0;
  }
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int first = (blockIdx.x * EL_SCORE_WAVES + wave) * 64;
  if (first >= C) return;                           // wave-uniform
  const int cand = first + lane;
  const int cc = cand < C ? cand : 0;
  const int ia = cc / side, ib = cc - ia * side;    // a + W, b + W
  const unsigned char *e = el_E + ia * P + ib;      // E[i + a][j + b] lies at e[i * P + j]
  const int count = min(max(a.occ[(size_t)s * (1 + a.Y) + 1 + k], 0), cells);
  const int *__restrict__ list = a.list + ((size_t)s * a.Y + k) * cells;       // wave-uniform: scalar loads
  const int L = a.L;
  int acc = 0;
  for (int t = 0; t < count; ++t) {
    const int w = list[t];
    const int i = w & 255, j = (w >> 8) & 255, q = (w >> 16) & 255;
    if (i >= G || j >= G) continue;                 // uniform; image never writes one
    const int ev = (int)e[i * P + j];
    const int d = abs(q - ev);
    acc += ev != 0 ? max(0, L - d) : 0;
  }
  if (cand < C) a.A[((size_t)s * a.Y + k) * C + cand] = acc;
}

// ---- choose: one workgroup per stream ---------------------------------------------------------------------------------------

struct ElChoose {
  int S, NS, Y, W, L, up_neg_y;
  float min_agreement, c;
  const int *found, *match;
  const int *A;                     // (S, Y, 2W+1, 2W+1)
  const int *occ;                   // (S, 1 + Y)
  const double *pose;               // (NS Y, 4, 4): [R(theta), 0], row shift * Y + k
  const double *T0;                 // (S, 4, 4): select's start pose
  int *record;                      // (S, 8): found, k, a, b, A, occ_Q, occ_E, 0
  double *T1;                       // (S, 4, 4)
};

__global__ __launch_bounds__(EL_CHOOSE_THREADS) void el_choose_kernel(ElChoose a) {
  __shared__ int red_v[EL_CHOOSE_THREADS];
  __shared__ int red_i[EL_CHOOSE_THREADS];
  __shared__ int chosen[4];                         // found, row of the pose table, a, b
  const int s = blockIdx.x, tid = threadIdx.x;
  const int side = 2 * a.W + 1, C = side * side, total = a.Y * C;
  const int shift = a.match[(size_t)s * LC_MATCH + 3];
  const bool matched = a.found[s] != 0 && shift >= 0 && shift < a.NS;
  int best = -1, at = total;
  if (matched) {
    const int *A = a.A + (size_t)s * total;
    for (int i = tid; i < total; i += EL_CHOOSE_THREADS) {          // ascending per thread: strict > keeps the lowest index
      const int v = A[i];
      if (v > best) {
        best = v;
        at = i;
      }
    }
  }
  red_v[tid] = best;
  red_i[tid] = at;
  __syncthreads();
  for (int half = EL_CHOOSE_THREADS / 2; half >= 1; half >>= 1) {
    if (tid < half) {
      const int ov = red_v[tid + half], oi = red_i[tid + half];
      if (ov > red_v[tid] || (ov == red_v[tid] && oi < red_i[tid])) {
        red_v[tid] = ov;
        red_i[tid] = oi;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    best = red_v[0];
    at = red_i[0];
    int *rec = a.record + (size_t)s * EL_RECORD;
    int ok = 0, k = 0, ia = a.W, ib = a.W, oq = 0, oe = 0;
    if (matched && at < total) {
      k = at / C;
      const int rest = at - k * C;
      ia = rest / side;
      ib = rest - ia * side;
      oq = a.occ[(size_t)s * (1 + a.Y) + 1 + k];
      oe = a.occ[(size_t)s * (1 + a.Y)];
      const float bound = a.min_agreement * (float)(a.L * min(oq, oe));
      ok = best > 0 && (float)best >= bound ? 1 : 0;
    } else {
      best = 0;
    }
    rec[0] = ok;
    rec[1] = k;
    rec[2] = ia - a.W;
    rec[3] = ib - a.W;
    rec[4] = best;
    rec[5] = oq;
    rec[6] = oe;
    rec[7] = 0;
    chosen[0] = ok;
    chosen[1] = matched ? shift * a.Y + k : 0;
    chosen[2] = ia - a.W;
    chosen[3] = ib - a.W;
  }
  __syncthreads();
  if (tid < 16) {
    double v = a.T0[(size_t)s * 16 + tid];          // not found: T0 to the bit, today's start
    if (chosen[0] != 0) {
      const int r = tid >> 2, c = tid & 3;
      v = a.pose[(size_t)chosen[1] * 16 + tid];
      if (c == 3 && r < 3) {
        const double ta = (double)chosen[2] * (double)a.c, tb = (double)chosen[3] * (double)a.c;
        const double tnb = (double)(-chosen[3]) * (double)a.c;
        v = a.up_neg_y ? (r == 0 ? tnb : r == 1 ? 0.0 : ta) : (r == 0 ? ta : r == 1 ? tb : 0.0);
      }
    }
    a.T1[(size_t)s * 16 + tid] = v;
  }
}

}  // namespace pwclo

using namespace pwclo;

static bool el_shape(const char *what, int S, int G, int Y, int W) {
  if (!(S >= 1 && S <= LC_MAX_STREAMS)) {
    set_error(PWCLO_EINVAL, "%s: S=%d streams outside [1, %d]", what, S, LC_MAX_STREAMS);
    return false;
  }
  if (!(G >= EL_MIN_CELLS && G <= EL_MAX_CELLS && G % 2 == 0) || !(Y >= 1 && Y <= EL_MAX_YAW && Y % 2 == 1) ||
      !(W >= 0 && W <= EL_MAX_WINDOW)) {
    set_error(PWCLO_EINVAL, "%s: cells=%d not even in [%d, %d], yaw candidates=%d not odd in [1, %d] or window=%d outside [0, %d]",
              what, G, EL_MIN_CELLS, EL_MAX_CELLS, Y, EL_MAX_YAW, W, EL_MAX_WINDOW);
    return false;
  }
  return true;
}

extern "C" void elevation_image_kernel_wrapper(int S, int n, int NS, int G, int Y, int up_neg_y, float z_offset,
                                               float cell_size, float z_step, const float *cloud, const float *staging,
                                               const int *lengths, const int *found, const int *match, const float *rot,
                                               void *img, int *occ, int *list) {
  if (!el_shape("elevation_image", S, G, Y, 0)) return;
  PWCLO_REQUIRE(n >= 1 && n <= (1 << 24), "elevation_image: n=%d points outside [1, 2^24]", n);
  PWCLO_REQUIRE(NS >= LC_MIN_SECTORS && NS <= LC_MAX_SECTORS, "elevation_image: sectors=%d outside [%d, %d]", NS,
                LC_MIN_SECTORS, LC_MAX_SECTORS);
  PWCLO_REQUIRE(cell_size > 0.f && cell_size <= 3.0e38f && z_step > 0.f && z_step <= 3.0e38f && z_offset >= -3.0e38f &&
                    z_offset <= 3.0e38f,
                "elevation_image: cell_size=%g and z_step=%g must be finite and > 0, z_offset=%g finite", cell_size, z_step,
                z_offset);
  PWCLO_REQUIRE(cloud && staging && found && match && rot && img && occ && list, "elevation_image: a null argument");
  ElImage a{S, n, NS, G, Y, up_neg_y != 0, z_offset, cell_size, z_step, cloud, staging, lengths, found, match, rot,
            (unsigned char *)img, occ, list};
  const int lds = (G * G + 4) * (int)sizeof(unsigned);
  if (lds > 64 * 1024) raise_lds_limit<el_image_kernel>(160 * 1024);
  hipLaunchKernelGGL(el_image_kernel, dim3(1 + Y, S), dim3(EL_IMAGE_THREADS), lds, current_stream(), a);
  check_launch("elevation_image");
}

extern "C" void elevation_score_kernel_wrapper(int S, int G, int Y, int W, int L, const int *found, const void *img,
                                               const int *occ, const int *list, int *A) {
  if (!el_shape("elevation_score", S, G, Y, W)) return;
  PWCLO_REQUIRE(L >= 1 && L <= 255, "elevation_score: tolerance=%d outside [1, 255]", L);
  PWCLO_REQUIRE(found && img && occ && list && A, "elevation_score: a null argument");
  ElScore a{S, G, Y, W, L, found, (const unsigned char *)img, occ, list, A};
  const int side = 2 * W + 1, P = G + 2 * W;
  const int lds = ceil_div(P * P, 16) * 16;
  hipLaunchKernelGGL(el_score_kernel, dim3(ceil_div(side * side, EL_SCORE_WAVES * 64), Y, S), dim3(EL_SCORE_WAVES * 64), lds,
                     current_stream(), a);
  check_launch("elevation_score");
}

extern "C" void elevation_choose_kernel_wrapper(int S, int NS, int Y, int W, int L, int up_neg_y, float min_agreement,
                                                float cell_size, const int *found, const int *match, const int *A,
                                                const int *occ, const double *pose, const double *T0, int *record,
                                                double *T1) {
  if (!el_shape("elevation_choose", S, EL_MIN_CELLS, Y, W)) return;
  PWCLO_REQUIRE(NS >= LC_MIN_SECTORS && NS <= LC_MAX_SECTORS, "elevation_choose: sectors=%d outside [%d, %d]", NS,
                LC_MIN_SECTORS, LC_MAX_SECTORS);
  PWCLO_REQUIRE(L >= 1 && L <= 255, "elevation_choose: tolerance=%d outside [1, 255]", L);
  PWCLO_REQUIRE(min_agreement >= 0.f && min_agreement <= 1.f && cell_size > 0.f && cell_size <= 3.0e38f,
                "elevation_choose: min_agreement=%g outside [0, 1] or cell_size=%g not finite and > 0", min_agreement,
                cell_size);
  PWCLO_REQUIRE(found && match && A && occ && pose && T0 && record && T1, "elevation_choose: a null argument");
  ElChoose a{S, NS, Y, W, L, up_neg_y != 0, min_agreement, cell_size, found, match, A, occ, pose, T0, record, T1};
  hipLaunchKernelGGL(el_choose_kernel, dim3(S), dim3(EL_CHOOSE_THREADS), 0, current_stream(), a);
  check_launch("elevation_choose");
}
