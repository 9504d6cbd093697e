// Training pose head with replayable dropout masks (pose_head.py, training.DropoutStream), gfx950.
//
// PW/pose_calculator.py:47-86 in train() mode, from the mask LOGITS:
//     p = softmax_n(logits);  pooled = sum_n emb p;  big = W_qt pooled + b_qt
//     big_q = dropout(big), big_t = dropout(big)                     (two independent masks, p = 0.5)
//     q = W_q big_q + b_q,  q / (sqrt(sum q^2 + 1e-10) + 1e-10);     t = W_t big_t + b_t
// On the module path torch runs that as softmax, multiply, sum, three matrix products, two dropouts, the norm and their
// backward: about forty small launches per head and step, four heads.  Here: 1 + 2 launches forward, 3 backward.
//   begin      one thread: state[2] = state[1]; state[1] += 1        (state = {seed, next step, step in flight})
//   rows  fwd  one wave per (b, c) row of N logits / values: online soft-max (running maximum, one read of the row)
//   cloud fwd  one workgroup per cloud, thread = hidden unit: 64 -> 256, the two keep bits, 256 -> 4 / 3, the norm
//   cloud bwd  one workgroup per cloud: norm, 4 / 3 -> 256 through the saved keep byte, 256 -> 64
//   param bwd  one thread per parameter value, summed over the batch in batch order (no floating-point atomics)
//   rows  bwd  elementwise: d_emb = g p, d_logits = g p (emb - pooled), p recomputed from the saved maximum and 1 / sum
// Keep bit of unit c of cloud b = top bit of Philox word 0 at counter (b * 256 + c, rank * 8 + head * 2 + branch, step, 3):
// a function of (seed, step, rank, head, branch, element) alone, so a captured graph replays it and any device repeats it.
// A kept value is multiplied by exactly 2.0f, a dropped one is +0.0f.  Built with -ffp-contract=off like every file here:
// products and sums are rounded separately, in the order written.
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "common.hpp"
#include "philox.hpp"

namespace pwclo {

constexpr int PH_IN = 64;      // channels of emb / logits
constexpr int PH_HID = 256;    // hidden units (conv1d_q_t)
constexpr int PH_THREADS = 256;

struct OpAddF32 { __device__ __forceinline__ float operator()(float a, float b) const { return a + b; } };
struct OpMaxNanF32 { __device__ __forceinline__ float operator()(float a, float b) const { return max_nan(a, b); } };

__global__ void pose_head_begin_kernel(long long *__restrict__ state) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const long long step = state[1];
    state[2] = step;
    state[1] = step + 1;
  }
}

// One wave per row.  Every lane keeps (m, s, w) = (running maximum, sum of exp(x - m), sum of exp(x - m) e) over its own
// elements and rescales them when a group of elements raises the maximum; the lanes are brought to the row maximum once
// and summed.  VEC: N % 4 == 0, so every row starts 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(PH_THREADS) void pose_head_rows_fwd_kernel(int rows, int N, const float *__restrict__ emb,
                                                                        const float *__restrict__ logits,
                                                                        float *__restrict__ rowmax, float *__restrict__ rinv,
                                                                        float *__restrict__ pooled) {
  const int row = (int)blockIdx.x * (PH_THREADS / WAVE) + (int)(threadIdx.x >> 6);
  if (row >= rows) return;                                 // wave-uniform
  const int lane = lane_id();
  const float *x = logits + (size_t)row * N, *e = emb + (size_t)row * N;
  float m = -FLT_MAX, s = 0.f, w = 0.f;
  if constexpr (VEC) {
    for (int i = lane * 4; i < N; i += WAVE * 4) {
      const float4 xv = *reinterpret_cast<const float4 *>(x + i), ev = *reinterpret_cast<const float4 *>(e + i);
      const float cm = max_nan(max_nan(xv.x, xv.y), max_nan(xv.z, xv.w));
      if (cm > m) {
        const float r = expf(m - cm);
        s = s * r; w = w * r; m = cm;
      }
      const float p0 = expf(xv.x - m), p1 = expf(xv.y - m), p2 = expf(xv.z - m), p3 = expf(xv.w - m);
      s = s + ((p0 + p1) + (p2 + p3));
      w = w + ((p0 * ev.x + p1 * ev.y) + (p2 * ev.z + p3 * ev.w));
    }
  } else {
    for (int i = lane; i < N; i += WAVE) {
      const float xv = x[i], ev = e[i];
      if (xv > m) {
        const float r = expf(m - xv);
        s = s * r; w = w * r; m = xv;
      }
      const float p = expf(xv - m);
      s = s + p;
      w = w + p * ev;
    }
  }
  const float M = wave_allreduce_f32(m, OpMaxNanF32());
  const float r = expf(m - M);                             // a lane without elements: exp(-FLT_MAX - M) = 0, times 0
  s = wave_allreduce_f32(s * r, OpAddF32());
  w = wave_allreduce_f32(w * r, OpAddF32());
  if (lane == 0) {
    rowmax[row] = M;
    rinv[row] = 1.0f / s;
    pooled[row] = w / s;
  }
}

// One workgroup per cloud, thread c = hidden unit c.
__global__ __launch_bounds__(PH_THREADS) void pose_head_cloud_fwd_kernel(
    const float *__restrict__ pooled, const float *__restrict__ w_qt, const float *__restrict__ b_qt,
    const float *__restrict__ w_q, const float *__restrict__ b_q, const float *__restrict__ w_t,
    const float *__restrict__ b_t, const long long *__restrict__ state, unsigned unit, float *__restrict__ big_out,
    unsigned char *__restrict__ keep_out, unsigned char *__restrict__ keep_log, float *__restrict__ q_raw,
    float *__restrict__ q, float *__restrict__ t) {
  __shared__ float sp[PH_IN];
  __shared__ float part[PH_THREADS / WAVE][8];
  const int b = blockIdx.x, c = threadIdx.x, lane = lane_id(), wave = c >> 6;
  if (c < PH_IN) sp[c] = pooled[(size_t)b * PH_IN + c];
  __syncthreads();
  const float *wr = w_qt + (size_t)c * PH_IN;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
  for (int k = 0; k < PH_IN; k += 4) {
    const float4 wv = *reinterpret_cast<const float4 *>(wr + k);
    a0 = a0 + wv.x * sp[k]; a1 = a1 + wv.y * sp[k + 1]; a2 = a2 + wv.z * sp[k + 2]; a3 = a3 + wv.w * sp[k + 3];
  }
  const float big = ((a0 + a1) + (a2 + a3)) + b_qt[c];
  const unsigned long long seed = (unsigned long long)state[0];
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32), step = (unsigned)state[2];
  const unsigned index = (unsigned)b * (unsigned)PH_HID + (unsigned)c;
  const bool kq = (philox_word(index, unit, step, PH_DROPOUT, k0, k1) >> 31) != 0u;
  const bool kt = (philox_word(index, unit + 1u, step, PH_DROPOUT, k0, k1) >> 31) != 0u;
  const unsigned char kb = (unsigned char)((kq ? 1 : 0) | (kt ? 2 : 0));
  const float bq = kq ? 2.0f * big : 0.0f, bt = kt ? 2.0f * big : 0.0f;
  big_out[(size_t)b * PH_HID + c] = big;
  keep_out[(size_t)b * PH_HID + c] = kb;
  if (keep_log != nullptr) keep_log[(size_t)b * PH_HID + c] = kb;
  float v[7];
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = w_q[j * PH_HID + c] * bq;
#pragma unroll
  for (int j = 0; j < 3; ++j) v[4 + j] = w_t[j * PH_HID + c] * bt;
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    v[j] = wave_allreduce_f32(v[j], OpAddF32());
    if (lane == 0) part[wave][j] = v[j];
  }
  __syncthreads();
  if (c == 0) {
    float o[7];
#pragma unroll
    for (int j = 0; j < 7; ++j)
      o[j] = ((part[0][j] + part[1][j]) + (part[2][j] + part[3][j])) + (j < 4 ? b_q[j] : b_t[j - 4]);
    const float ss = (o[0] * o[0] + o[1] * o[1]) + (o[2] * o[2] + o[3] * o[3]);
    const float d = sqrtf(ss + 1e-10f) + 1e-10f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      q_raw[(size_t)b * 4 + j] = o[j];
      q[(size_t)b * 4 + j] = o[j] / d;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) t[(size_t)b * 3 + j] = o[4 + j];
  }
}

// One workgroup per cloud: (g_q, g_t) -> g_qraw (B,4), g_big (B,256), g_pooled (B,64).
__global__ __launch_bounds__(PH_THREADS) void pose_head_cloud_bwd_kernel(
    const float *__restrict__ g_q, const float *__restrict__ g_t, const float *__restrict__ q_raw,
    const unsigned char *__restrict__ keep, const float *__restrict__ w_qt, const float *__restrict__ w_q,
    const float *__restrict__ w_t, float *__restrict__ g_qraw, float *__restrict__ g_big, float *__restrict__ g_pooled) {
  __shared__ float sg[PH_HID];
  __shared__ float part[PH_THREADS / PH_IN][PH_IN];
  __shared__ float gq[4];
  const int b = blockIdx.x, c = threadIdx.x;
  if (c == 0) {
    float qv[4], g[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { qv[j] = q_raw[(size_t)b * 4 + j]; g[j] = g_q[(size_t)b * 4 + j]; }
    // y = q / d, d = r + 1e-10, r = sqrt(sum q^2 + 1e-10):  dq_j = g_j / d - (g . q) / d^2 * q_j / r
    const float ss = (qv[0] * qv[0] + qv[1] * qv[1]) + (qv[2] * qv[2] + qv[3] * qv[3]);
    const float r = sqrtf(ss + 1e-10f), d = r + 1e-10f;
    const float dot = (g[0] * qv[0] + g[1] * qv[1]) + (g[2] * qv[2] + g[3] * qv[3]);
    const float f = dot / (d * d);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float v = g[j] / d - f * (qv[j] / r);
      gq[j] = v;
      g_qraw[(size_t)b * 4 + j] = v;
    }
  }
  __syncthreads();
  const float t0 = g_t[(size_t)b * 3], t1 = g_t[(size_t)b * 3 + 1], t2 = g_t[(size_t)b * 3 + 2];
  const float aq = (w_q[c] * gq[0] + w_q[PH_HID + c] * gq[1]) + (w_q[2 * PH_HID + c] * gq[2] + w_q[3 * PH_HID + c] * gq[3]);
  const float at = (w_t[c] * t0 + w_t[PH_HID + c] * t1) + w_t[2 * PH_HID + c] * t2;
  const unsigned char kb = keep[(size_t)b * PH_HID + c];
  const float g = ((kb & 1) ? 2.0f * aq : 0.0f) + ((kb & 2) ? 2.0f * at : 0.0f);
  sg[c] = g;
  g_big[(size_t)b * PH_HID + c] = g;
  __syncthreads();
  const int k = c & (PH_IN - 1), quarter = c >> 6;         // 64 hidden units per quarter, consecutive k: coalesced rows
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 4
  for (int i = 0; i < PH_IN; i += 4) {
    const int h = quarter * PH_IN + i;
    a0 = a0 + w_qt[(size_t)h * PH_IN + k] * sg[h];
    a1 = a1 + w_qt[(size_t)(h + 1) * PH_IN + k] * sg[h + 1];
    a2 = a2 + w_qt[(size_t)(h + 2) * PH_IN + k] * sg[h + 2];
    a3 = a3 + w_qt[(size_t)(h + 3) * PH_IN + k] * sg[h + 3];
  }
  part[quarter][k] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (c < PH_IN) g_pooled[(size_t)b * PH_IN + c] = (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]);
}

constexpr int PH_N_WQT = PH_HID * PH_IN, PH_N_WQ = 4 * PH_HID, PH_N_WT = 3 * PH_HID;
constexpr int PH_PARAM_VALUES = PH_N_WQT + PH_HID + PH_N_WQ + 4 + PH_N_WT + 3;

// One thread per parameter value; the batch is summed in batch order.  A dropped unit adds nothing, so its column of
// d_w_q / d_w_t is exactly +0.0 when every cloud of the batch drops it.
__global__ __launch_bounds__(PH_THREADS) void pose_head_param_bwd_kernel(
    int B, const float *__restrict__ pooled, const float *__restrict__ big, const unsigned char *__restrict__ keep,
    const float *__restrict__ g_big, const float *__restrict__ g_qraw, const float *__restrict__ g_t,
    float *__restrict__ d_w_qt, float *__restrict__ d_b_qt, float *__restrict__ d_w_q, float *__restrict__ d_b_q,
    float *__restrict__ d_w_t, float *__restrict__ d_b_t) {
  int i = (int)blockIdx.x * PH_THREADS + (int)threadIdx.x;
  if (i >= PH_PARAM_VALUES) return;
  float acc = 0.f;
  if (i < PH_N_WQT) {
    const int c = i >> 6, k = i & (PH_IN - 1);
    for (int b = 0; b < B; ++b) acc = acc + g_big[(size_t)b * PH_HID + c] * pooled[(size_t)b * PH_IN + k];
    d_w_qt[i] = acc;
    return;
  }
  i -= PH_N_WQT;
  if (i < PH_HID) {
    for (int b = 0; b < B; ++b) acc = acc + g_big[(size_t)b * PH_HID + i];
    d_b_qt[i] = acc;
    return;
  }
  i -= PH_HID;
  if (i < PH_N_WQ) {
    const int j = i >> 8, c = i & (PH_HID - 1);
    for (int b = 0; b < B; ++b)
      if (keep[(size_t)b * PH_HID + c] & 1) acc = acc + g_qraw[(size_t)b * 4 + j] * (2.0f * big[(size_t)b * PH_HID + c]);
    d_w_q[i] = acc;
    return;
  }
  i -= PH_N_WQ;
  if (i < 4) {
    for (int b = 0; b < B; ++b) acc = acc + g_qraw[(size_t)b * 4 + i];
    d_b_q[i] = acc;
    return;
  }
  i -= 4;
  if (i < PH_N_WT) {
    const int j = i >> 8, c = i & (PH_HID - 1);
    for (int b = 0; b < B; ++b)
      if (keep[(size_t)b * PH_HID + c] & 2) acc = acc + g_t[(size_t)b * 3 + j] * (2.0f * big[(size_t)b * PH_HID + c]);
    d_w_t[i] = acc;
    return;
  }
  i -= PH_N_WT;
  for (int b = 0; b < B; ++b) acc = acc + g_t[(size_t)b * 3 + i];
  d_b_t[i] = acc;
}

// Elementwise over the rows * N values.  VEC: N % 4 == 0, four values of one row per thread.
template <bool VEC>
__global__ __launch_bounds__(PH_THREADS) void pose_head_rows_bwd_kernel(long long total, int N, const float *__restrict__ emb,
                                                                        const float *__restrict__ logits,
                                                                        const float *__restrict__ rowmax,
                                                                        const float *__restrict__ rinv,
                                                                        const float *__restrict__ pooled,
                                                                        const float *__restrict__ g_pooled,
                                                                        float *__restrict__ d_emb, float *__restrict__ d_logits) {
  const long long i = ((long long)blockIdx.x * PH_THREADS + threadIdx.x) * (VEC ? 4 : 1);
  if (i >= total) return;
  const long long row = i / N;
  const float M = rowmax[row], ri = rinv[row], out = pooled[row], g = g_pooled[row];
  if constexpr (VEC) {
    const float4 xv = *reinterpret_cast<const float4 *>(logits + i), ev = *reinterpret_cast<const float4 *>(emb + i);
    const float x[4] = {xv.x, xv.y, xv.z, xv.w}, e[4] = {ev.x, ev.y, ev.z, ev.w};
    float de[4], dx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      de[j] = g * (expf(x[j] - M) * ri);
      dx[j] = de[j] * (e[j] - out);
    }
    *reinterpret_cast<float4 *>(d_emb + i) = make_float4(de[0], de[1], de[2], de[3]);
    *reinterpret_cast<float4 *>(d_logits + i) = make_float4(dx[0], dx[1], dx[2], dx[3]);
  } else {
    const float de = g * (expf(logits[i] - M) * ri);
    d_emb[i] = de;
    d_logits[i] = de * (emb[i] - out);
  }
}

static inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace pwclo

using namespace pwclo;

extern "C" void pose_head_train_begin_kernel_wrapper(long long *state) {
  PWCLO_REQUIRE(state != nullptr, "pose_head_train_begin: the state is required%s", "");
  hipLaunchKernelGGL(pose_head_begin_kernel, dim3(1), dim3(1), 0, current_stream(), state);
  check_launch("pose_head_train_begin");
}

extern "C" void pose_head_train_forward_kernel_wrapper(int B, int N, const float *emb, const float *logits, const float *w_qt,
                                                       const float *b_qt, const float *w_q, const float *b_q,
                                                       const float *w_t, const float *b_t, const long long *state, int rank,
                                                       int head, float *rowmax, float *rinv, float *pooled, float *big,
                                                       unsigned char *keep, unsigned char *keep_log, float *q_raw, float *q,
                                                       float *t) {
  PWCLO_REQUIRE(B >= 1 && B <= (1 << 20) && N >= 1 && N <= (1 << 24), "pose_head_train_forward: B=%d N=%d out of range", B, N);
  PWCLO_REQUIRE((long long)B * PH_IN * N < (1ll << 38), "pose_head_train_forward: %lld values exceed the grid",
                (long long)B * PH_IN * N);
  PWCLO_REQUIRE(rank >= 0 && rank < (1 << 28) && head >= 0 && head < 4, "pose_head_train_forward: rank=%d head=%d", rank, head);
  PWCLO_REQUIRE(emb && logits && w_qt && b_qt && w_q && b_q && w_t && b_t && state && rowmax && rinv && pooled && big && keep &&
                q_raw && q && t, "pose_head_train_forward: every pointer but keep_log is required%s", "");
  PWCLO_REQUIRE(aligned16(emb) && aligned16(logits) && aligned16(w_qt),
                "pose_head_train_forward: emb, logits and w_qt must be 16-byte aligned%s", "");
  const int rows = B * PH_IN;
  const dim3 grid((unsigned)ceil_div(rows, PH_THREADS / WAVE));
  if (N % 4 == 0)
    hipLaunchKernelGGL(pose_head_rows_fwd_kernel<true>, grid, dim3(PH_THREADS), 0, current_stream(), rows, N, emb, logits,
                       rowmax, rinv, pooled);
  else
    hipLaunchKernelGGL(pose_head_rows_fwd_kernel<false>, grid, dim3(PH_THREADS), 0, current_stream(), rows, N, emb, logits,
                       rowmax, rinv, pooled);
  hipLaunchKernelGGL(pose_head_cloud_fwd_kernel, dim3((unsigned)B), dim3(PH_THREADS), 0, current_stream(), pooled, w_qt, b_qt,
                     w_q, b_q, w_t, b_t, state, (unsigned)rank * 8u + (unsigned)head * 2u, big, keep, keep_log, q_raw, q, t);
  check_launch("pose_head_train_forward");
}

extern "C" void pose_head_train_backward_kernel_wrapper(int B, int N, const float *emb, const float *logits, const float *w_qt,
                                                        const float *w_q, const float *w_t, const float *rowmax,
                                                        const float *rinv, const float *pooled, const float *big,
                                                        const unsigned char *keep, const float *q_raw, const float *g_q,
                                                        const float *g_t, float *g_qraw, float *g_big, float *g_pooled,
                                                        float *d_emb, float *d_logits, float *d_w_qt, float *d_b_qt,
                                                        float *d_w_q, float *d_b_q, float *d_w_t, float *d_b_t) {
  PWCLO_REQUIRE(B >= 1 && B <= (1 << 20) && N >= 1 && N <= (1 << 24), "pose_head_train_backward: B=%d N=%d out of range", B, N);
  PWCLO_REQUIRE((long long)B * PH_IN * N < (1ll << 38), "pose_head_train_backward: %lld values exceed the grid",
                (long long)B * PH_IN * N);
  PWCLO_REQUIRE(emb && logits && w_qt && w_q && w_t && rowmax && rinv && pooled && big && keep && q_raw && g_q && g_t &&
                g_qraw && g_big && g_pooled && d_emb && d_logits && d_w_qt && d_b_qt && d_w_q && d_b_q && d_w_t && d_b_t,
                "pose_head_train_backward: every pointer is required%s", "");
  PWCLO_REQUIRE(aligned16(emb) && aligned16(logits) && aligned16(d_emb) && aligned16(d_logits),
                "pose_head_train_backward: emb, logits and their gradients must be 16-byte aligned%s", "");
  hipLaunchKernelGGL(pose_head_cloud_bwd_kernel, dim3((unsigned)B), dim3(PH_THREADS), 0, current_stream(), g_q, g_t, q_raw,
                     keep, w_qt, w_q, w_t, g_qraw, g_big, g_pooled);
  hipLaunchKernelGGL(pose_head_param_bwd_kernel, dim3((unsigned)ceil_div(PH_PARAM_VALUES, PH_THREADS)), dim3(PH_THREADS), 0,
                     current_stream(), B, pooled, big, keep, g_big, g_qraw, g_t, d_w_qt, d_b_qt, d_w_q, d_b_q, d_w_t, d_b_t);
  const long long total = (long long)B * PH_IN * N;
  if (N % 4 == 0)
    hipLaunchKernelGGL(pose_head_rows_bwd_kernel<true>, dim3((unsigned)((total / 4 + PH_THREADS - 1) / PH_THREADS)),
                       dim3(PH_THREADS), 0, current_stream(), total, N, emb, logits, rowmax, rinv, pooled, g_pooled, d_emb,
                       d_logits);
  else
    hipLaunchKernelGGL(pose_head_rows_bwd_kernel<false>, dim3((unsigned)((total + PH_THREADS - 1) / PH_THREADS)),
                       dim3(PH_THREADS), 0, current_stream(), total, N, emb, logits, rowmax, rinv, pooled, g_pooled, d_emb,
                       d_logits);
  check_launch("pose_head_train_backward");
}
