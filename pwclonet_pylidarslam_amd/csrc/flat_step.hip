// Flat gradient bucket and Adam over a list of fp32 tensors (flat_step.FlatAdam).  The data-parallel
// step's two halves around its one collective:
//   flat_pack   gathers the gradients (pointer, count, bucket offset) into ONE buffer, scaled by 1 / world, zero padding
//               between tensors, and counts the non-finite inputs into the bucket's last value (as fp32: the SUM
//               all-reduce of the bucket then hands every rank the same verdict);
//   flat_adam   torch.optim.Adam / AdamW over the same list (parameter pointers in the table; gradient and both moments
//               flat at the bucket offsets), step counter and learning rate in device memory, the whole update skipped
//               when the count is not zero.
// The tensor list travels BY VALUE in the kernel arguments, FLAT_ENTRIES tensors per launch and as many launches as the
// list needs (the multi-tensor-apply scheme): a captured graph bakes the list in and replays without host memory.
// Every value is stored by ordinary vector stores; the counter is moved by a one-thread launch of its own.
#include <stdint.h>

#include "common.hpp"

namespace pwclo {

constexpr int FLAT_ENTRIES = 128;       // tensors per launch: 128 * 16 B = 2 KiB of kernel arguments
constexpr unsigned FLAT_ALIGN = 64u;    // values: every bucket offset is a multiple (256 B)
constexpr int FLAT_THREADS = 256;
constexpr int FLAT_QUAD = 4 * FLAT_THREADS;   // values one workgroup covers per sweep
constexpr int FLAT_MAX_BLOCKS = 64;     // workgroups per tensor (grid.x); longer tensors are walked in sweeps

struct FlatEntry {
  float *ptr;          // the tensor (gradient for pack, parameter for adam); 4-byte aligned is enough
  unsigned offset;     // first value in the bucket, a multiple of FLAT_ALIGN
  unsigned count;      // values
};
struct FlatTable {
  FlatEntry e[FLAT_ENTRIES];
};

__device__ __forceinline__ int nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u ? 1 : 0; }

__global__ void flat_slot_zero_kernel(float *slot) {
  if (threadIdx.x == 0) *slot = 0.0f;
}

// grid (sweep workgroups, tensors of this launch).  Thread t of a sweep owns values [4t, 4t + 4) of the tensor's padded
// span (count rounded up to FLAT_ALIGN): values past count are written as zero, so the padding needs no pass of its own.
__global__ __launch_bounds__(FLAT_THREADS) void flat_pack_kernel(FlatTable tab, float scale, float *bucket, float *slot) {
  const FlatEntry e = tab.e[blockIdx.y];
  const unsigned span = (e.count + (FLAT_ALIGN - 1u)) & ~(FLAT_ALIGN - 1u);
  const bool vec = (reinterpret_cast<uintptr_t>(e.ptr) & 15u) == 0u;
  float *dst = bucket + e.offset;
  int bad = 0;
  for (unsigned i = (blockIdx.x * FLAT_THREADS + threadIdx.x) * 4u; i < span; i += gridDim.x * FLAT_QUAD) {
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (vec && i + 3u < e.count) {
      v = *reinterpret_cast<const float4 *>(e.ptr + i);
    } else {
      if (i < e.count) v.x = e.ptr[i];
      if (i + 1u < e.count) v.y = e.ptr[i + 1u];
      if (i + 2u < e.count) v.z = e.ptr[i + 2u];
      if (i + 3u < e.count) v.w = e.ptr[i + 3u];
    }
    bad += (nonfinite(v.x) + nonfinite(v.y)) + (nonfinite(v.z) + nonfinite(v.w));
    v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
    *reinterpret_cast<float4 *>(dst + i) = v;
  }
  if (__ballot(bad != 0) != 0ull) {                      // rare: one atomic per wave that saw one (integers: exact below 2^24)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
    if ((threadIdx.x & 63) == 0) atomicAdd(slot, (float)bad);
  }
}

// One thread, BEFORE the update launches: the only writer of the counter and of coef, which those launches only read.
// coef = {apply (1 / 0), lr / (1 - beta1^t), sqrt(1 - beta2^t), lr}.
// skipped (nullable): the cumulative count of steps not applied, which no pack resets.
__global__ void flat_adam_head_kernel(const float *__restrict__ slot, long long *__restrict__ step,
                                      const double *__restrict__ lr, double *__restrict__ coef, double beta1, double beta2,
                                      long long *__restrict__ skipped) {
  if (threadIdx.x != 0) return;
  if (!(*slot == 0.0f)) {                                // non-finite gradients somewhere: this step is not applied
    coef[0] = 0.0;
    if (skipped != nullptr) *skipped = *skipped + 1;
    return;
  }
  const long long t = *step + 1;
  *step = t;
  const double l = *lr;
  coef[0] = 1.0;
  coef[1] = l / (1.0 - pow(beta1, (double)t));
  coef[2] = sqrt(1.0 - pow(beta2, (double)t));
  coef[3] = l;
}

// torch/optim/adam.py _single_tensor_adam (amsgrad = maximize = False), evaluated per value in fp64 from the fp32 inputs
// and rounded ONCE per stored value (parameter, exp_avg, exp_avg_sq).
__device__ __forceinline__ void adam_value(bool decoupled, double g, float &p, float &m, float &v, double step_size,
                                           double bc2_sqrt, double lr, double beta1, double beta2, double eps, double wd) {
  double pd = p;
  if (decoupled)
    pd *= 1.0 - lr * wd;
  else
    g += wd * pd;
  const double md = m + (g - m) * (1.0 - beta1);
  const double vd = beta2 * v + (1.0 - beta2) * g * g;
  const double denom = sqrt(vd) / bc2_sqrt + eps;
  pd -= step_size * (md / denom);
  p = (float)pd;
  m = (float)md;
  v = (float)vd;
}

template <bool DECOUPLED>
__global__ __launch_bounds__(FLAT_THREADS) void flat_adam_kernel(FlatTable tab, const float *__restrict__ grad,
                                                                  float *__restrict__ exp_avg, float *__restrict__ exp_avg_sq,
                                                                  const double *__restrict__ coef, double beta1, double beta2,
                                                                  double eps, double wd) {
  if (coef[0] == 0.0) return;
  const double step_size = coef[1], bc2_sqrt = coef[2], lr = coef[3];
  const FlatEntry e = tab.e[blockIdx.y];
  const bool vec = (reinterpret_cast<uintptr_t>(e.ptr) & 15u) == 0u;
  const float *g = grad + e.offset;
  float *m = exp_avg + e.offset, *v = exp_avg_sq + e.offset;
  // the flat buffers are read and written in whole quads: the padded span of a tensor is a multiple of FLAT_ALIGN, its
  // padding holds zeros in all three and keeps them (g = 0, p = 0 there)
  for (unsigned i = (blockIdx.x * FLAT_THREADS + threadIdx.x) * 4u; i < e.count; i += gridDim.x * FLAT_QUAD) {
    const bool whole = vec && i + 3u < e.count;
    const float4 g4 = *reinterpret_cast<const float4 *>(g + i);
    float4 m4 = *reinterpret_cast<const float4 *>(m + i), v4 = *reinterpret_cast<const float4 *>(v + i);
    float4 p4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (whole) {
      p4 = *reinterpret_cast<const float4 *>(e.ptr + i);
    } else {
      p4.x = e.ptr[i];
      if (i + 1u < e.count) p4.y = e.ptr[i + 1u];
      if (i + 2u < e.count) p4.z = e.ptr[i + 2u];
      if (i + 3u < e.count) p4.w = e.ptr[i + 3u];
    }
    adam_value(DECOUPLED, g4.x, p4.x, m4.x, v4.x, step_size, bc2_sqrt, lr, beta1, beta2, eps, wd);
    adam_value(DECOUPLED, g4.y, p4.y, m4.y, v4.y, step_size, bc2_sqrt, lr, beta1, beta2, eps, wd);
    adam_value(DECOUPLED, g4.z, p4.z, m4.z, v4.z, step_size, bc2_sqrt, lr, beta1, beta2, eps, wd);
    adam_value(DECOUPLED, g4.w, p4.w, m4.w, v4.w, step_size, bc2_sqrt, lr, beta1, beta2, eps, wd);
    *reinterpret_cast<float4 *>(m + i) = m4;
    *reinterpret_cast<float4 *>(v + i) = v4;
    if (whole) {
      *reinterpret_cast<float4 *>(e.ptr + i) = p4;
    } else {
      e.ptr[i] = p4.x;
      if (i + 1u < e.count) e.ptr[i + 1u] = p4.y;
      if (i + 2u < e.count) e.ptr[i + 2u] = p4.z;
      if (i + 3u < e.count) e.ptr[i + 3u] = p4.w;
    }
  }
}

// Checks the list against the bucket and fills the tables of every launch; false (and a sticky error) when it does not fit.
static bool flat_tables(const char *what, int n, void *const *tensors, const long long *counts, const long long *offsets,
                        long long total, FlatTable *tabs, unsigned *max_span) {
  const long long slot = total - 1;
  for (int t = 0; t < n; ++t) {
    const long long c = counts[t], o = offsets[t], span = (c + (FLAT_ALIGN - 1)) / FLAT_ALIGN * FLAT_ALIGN;
    if (c < 0 || o < 0 || o % FLAT_ALIGN != 0 || o + span > slot) {
      set_error(PWCLO_EINVAL, "%s: tensor %d (count %lld, offset %lld) does not fit a bucket of %lld values with offsets "
                "aligned to %u (the last value is the non-finite count)", what, t, c, o, total, FLAT_ALIGN);
      return false;
    }
    if (c > 0 && (tensors[t] == nullptr || (reinterpret_cast<uintptr_t>(tensors[t]) & 3u) != 0u)) {
      set_error(PWCLO_EINVAL, "%s: tensor %d is NULL or not 4-byte aligned", what, t);
      return false;
    }
    FlatEntry &e = tabs[t / FLAT_ENTRIES].e[t % FLAT_ENTRIES];
    e.ptr = reinterpret_cast<float *>(tensors[t]);
    e.offset = (unsigned)o;
    e.count = (unsigned)c;
    unsigned &ms = max_span[t / FLAT_ENTRIES];
    ms = span > ms ? (unsigned)span : ms;
  }
  return true;
}

static dim3 flat_grid(unsigned max_span, int entries) {
  const unsigned bx = (max_span + FLAT_QUAD - 1) / FLAT_QUAD;
  return dim3(bx < 1u ? 1u : (bx > (unsigned)FLAT_MAX_BLOCKS ? (unsigned)FLAT_MAX_BLOCKS : bx), (unsigned)entries);
}

constexpr int FLAT_MAX_TENSORS = 32 * FLAT_ENTRIES;      // the tables of one call (64 KiB) live on the launcher's stack

}  // namespace pwclo

using namespace pwclo;

#define FLAT_COMMON_CHECKS(what)                                                                                           \
  PWCLO_REQUIRE(n >= 0 && n <= FLAT_MAX_TENSORS, what ": n=%d outside [0, %d]", n, FLAT_MAX_TENSORS);                      \
  PWCLO_REQUIRE(total >= 1 && total - 1 < (1ll << 31), what ": total=%lld outside [1, 2^31]", total);                      \
  PWCLO_REQUIRE(n == 0 || (tensors != nullptr && counts != nullptr && offsets != nullptr),                                 \
                what ": tensors, counts and offsets are required%s", "");                                                  \
  PWCLO_REQUIRE(bucket != nullptr && (reinterpret_cast<uintptr_t>(bucket) & 15u) == 0u,                                    \
                what ": the bucket must be 16-byte aligned%s", "")

extern "C" int flat_step_entries_per_launch(void) { return FLAT_ENTRIES; }

extern "C" void flat_pack_kernel_wrapper(int n, void *const *tensors, const long long *counts, const long long *offsets,
                                         float scale, float *bucket, long long total) {
  FLAT_COMMON_CHECKS("flat_pack");
  const int launches = (n + FLAT_ENTRIES - 1) / FLAT_ENTRIES;
  FlatTable tabs[FLAT_MAX_TENSORS / FLAT_ENTRIES] = {};
  unsigned max_span[FLAT_MAX_TENSORS / FLAT_ENTRIES] = {};
  if (!flat_tables("flat_pack", n, tensors, counts, offsets, total, tabs, max_span)) return;
  float *slot = bucket + (total - 1);
  hipLaunchKernelGGL(flat_slot_zero_kernel, dim3(1), dim3(64), 0, current_stream(), slot);
  for (int l = 0; l < launches; ++l) {
    const int entries = n - l * FLAT_ENTRIES < FLAT_ENTRIES ? n - l * FLAT_ENTRIES : FLAT_ENTRIES;
    hipLaunchKernelGGL(flat_pack_kernel, flat_grid(max_span[l], entries), dim3(FLAT_THREADS), 0, current_stream(), tabs[l],
                       scale, bucket, slot);
  }
  check_launch("flat_pack");
}

static void flat_adam(int n, void *const *tensors, const long long *counts, const long long *offsets, const float *bucket,
                      float *exp_avg, float *exp_avg_sq, long long total, long long *step, const double *lr, double *coef,
                      double beta1, double beta2, double eps, double weight_decay, int decoupled, long long *skipped) {
  FLAT_COMMON_CHECKS("flat_adam");
  PWCLO_REQUIRE(exp_avg != nullptr && exp_avg_sq != nullptr && (reinterpret_cast<uintptr_t>(exp_avg) & 15u) == 0u &&
                (reinterpret_cast<uintptr_t>(exp_avg_sq) & 15u) == 0u,
                "flat_adam: exp_avg and exp_avg_sq (total values each) must be 16-byte aligned%s", "");
  PWCLO_REQUIRE(step != nullptr && lr != nullptr && coef != nullptr, "flat_adam: step, lr and coef are required%s", "");
  PWCLO_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 && weight_decay >= 0.0,
                "flat_adam: betas (%g, %g) must lie in [0, 1), eps %g and weight_decay %g must not be negative", beta1, beta2,
                eps, weight_decay);
  const int launches = (n + FLAT_ENTRIES - 1) / FLAT_ENTRIES;
  FlatTable tabs[FLAT_MAX_TENSORS / FLAT_ENTRIES] = {};
  unsigned max_span[FLAT_MAX_TENSORS / FLAT_ENTRIES] = {};
  if (!flat_tables("flat_adam", n, tensors, counts, offsets, total, tabs, max_span)) return;
  hipLaunchKernelGGL(flat_adam_head_kernel, dim3(1), dim3(64), 0, current_stream(), bucket + (total - 1), step, lr, coef,
                     beta1, beta2, skipped);
  for (int l = 0; l < launches; ++l) {
    const int entries = n - l * FLAT_ENTRIES < FLAT_ENTRIES ? n - l * FLAT_ENTRIES : FLAT_ENTRIES;
    const dim3 grid = flat_grid(max_span[l], entries);
    if (decoupled)
      hipLaunchKernelGGL(flat_adam_kernel<true>, grid, dim3(FLAT_THREADS), 0, current_stream(), tabs[l], bucket, exp_avg,
                         exp_avg_sq, coef, beta1, beta2, eps, weight_decay);
    else
      hipLaunchKernelGGL(flat_adam_kernel<false>, grid, dim3(FLAT_THREADS), 0, current_stream(), tabs[l], bucket, exp_avg,
                         exp_avg_sq, coef, beta1, beta2, eps, weight_decay);
  }
  check_launch("flat_adam");
}

extern "C" void flat_adam_kernel_wrapper(int n, void *const *tensors, const long long *counts, const long long *offsets,
                                         const float *bucket, float *exp_avg, float *exp_avg_sq, long long total,
                                         long long *step, const double *lr, double *coef, double beta1, double beta2,
                                         double eps, double weight_decay, int decoupled) {
  flat_adam(n, tensors, counts, offsets, bucket, exp_avg, exp_avg_sq, total, step, lr, coef, beta1, beta2, eps, weight_decay,
            decoupled, nullptr);
}

extern "C" void flat_adam_skipped_kernel_wrapper(int n, void *const *tensors, const long long *counts,
                                                 const long long *offsets, const float *bucket, float *exp_avg,
                                                 float *exp_avg_sq, long long total, long long *step, const double *lr,
                                                 double *coef, double beta1, double beta2, double eps, double weight_decay,
                                                 int decoupled, long long *skipped) {
  PWCLO_REQUIRE(skipped != nullptr, "flat_adam_skipped: skipped is required%s", "");
  flat_adam(n, tensors, counts, offsets, bucket, exp_avg, exp_avg_sq, total, step, lr, coef, beta1, beta2, eps, weight_decay,
            decoupled, skipped);
}
