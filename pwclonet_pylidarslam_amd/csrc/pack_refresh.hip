// In-place refresh of the packed eval-mode weights (pack_plan.PackPlan, fused.FusedPWCLONet.refresh).
// ONE launch redoes what fused.py does per layer with a few dozen torch ops -- fold_conv_bn, column slice, row padding,
// pack_layer -- for every packed layer of the network, reading the live module tensors and writing the packed buffers
// where they are, so captured graphs that read those buffers keep working.  The jobs (include/pwclo_ops.h: PwcloPackJob)
// live in a device table recorded at pack time; the grid runs over (job, tile), a tile being one (o, m) fp32 operand tile,
// one (o, mp) reduced-format tile, or the job's bias vector.  One wave per tile, lane = the MFMA lane the values are for.
// Every destination element has exactly one writer; all stores are ordinary vector stores.
// The result is bit for bit pack_layer(*fold_conv_bn(layer)): the fold is evaluated in fp64 in fold_conv_bn's order and
// rounded to fp32 once, bf16 is round to nearest even, the bf16x3 residuals are fp32 differences.
#include <stdint.h>

#include "common.hpp"

#pragma clang fp contract(off)   // the library's build flag already says so; this file must not depend on it

namespace pwclo {

constexpr int PACK_FMT_F32 = 0, PACK_FMT_BF16X3 = 1;   // fused.py: WFMT_*; 2 = bf16, one term per weight

// Output channel held by physical row `prow` of the job (pack_layer's kmajor_out: channel c sits on row 4 * (c % 4) + c / 4,
// a 4 x 4 transpose and so its own inverse), or -1 for a padding row.
__device__ __forceinline__ int pack_channel(const PwcloPackJob &j, int prow) {
  const int c = j.kmajor ? 4 * (prow & 3) + (prow >> 2) : prow;
  return c < j.cout ? c : -1;
}

// gamma / sqrt(var + eps) of channel c in fp64 (fold_conv_bn: `s`); 1 without BatchNorm.
__device__ __forceinline__ double pack_scale(const PwcloPackJob &j, int c) {
  return (double)j.gamma[c] / sqrt((double)j.var[c] + j.eps);
}

// Folded weight of (physical row, physical input channel): 0 for padding rows and padding channels.
__device__ __forceinline__ float pack_weight(const PwcloPackJob &j, int prow, int pch) {
  const int c = pack_channel(j, prow);
  if (c < 0) return 0.0f;
  const int col = j.phys_map[pch];
  if (col < 0) return 0.0f;
  double w = (double)j.w[(long long)c * j.cin + (j.col0 + col)];
  if (j.var != nullptr) w = w * pack_scale(j, c);
  return (float)w;
}

__device__ __forceinline__ float pack_bias(const PwcloPackJob &j, int prow) {
  const int c = pack_channel(j, prow);
  if (c < 0 || !j.use_bias) return 0.0f;
  double b = j.conv_bias != nullptr ? (double)j.conv_bias[c] : 0.0;
  if (j.var != nullptr) b = (b - (double)j.mean[c]) * pack_scale(j, c) + (double)j.beta[c];
  return (float)b;
}

// fp32 -> bf16 bits, round to nearest even (NaN -> the quiet NaN torch writes).
__device__ __forceinline__ unsigned bf16_bits(float x) {
  const unsigned u = __float_as_uint(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ float bf16_value(unsigned bits) { return __uint_as_float(bits << 16); }

__global__ __launch_bounds__(64) void pack_layers_kernel(const PwcloPackJob *__restrict__ jobs, int njobs) {
  const int tile = blockIdx.x;
  int lo = 0, hi = njobs - 1;                      // the last job whose first tile is <= tile
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
  }
  const PwcloPackJob j = jobs[lo];
  const int lane = threadIdx.x, row = lane & 15, g = lane >> 4;
  const int cols = j.fmt == PACK_FMT_F32 ? j.nbi : j.nbi / 2;          // tiles per output block
  const int tile_floats = j.fmt == PACK_FMT_BF16X3 ? 768 : 256;
  const int t = tile - j.tile0;
  if (t >= j.nbo * cols) {                         // the job's last tile: 16 * nbo fp32 biases behind the operand tiles
    if (t > j.nbo * cols) return;
    float *bias = j.dst + (long long)j.nbo * cols * tile_floats;
    for (int i = lane; i < 16 * j.nbo; i += 64) bias[i] = pack_bias(j, i);
    return;
  }
  const int o = t / cols, m = t - o * cols, prow = 16 * o + row;
  float *dst = j.dst + (long long)t * tile_floats + 4 * lane;
  if (j.fmt == PACK_FMT_F32) {                     // [lane][4]: element r = physical channel 16 m + 4 g + r
    float4 v;
    v.x = pack_weight(j, prow, 16 * m + 4 * g + 0);
    v.y = pack_weight(j, prow, 16 * m + 4 * g + 1);
    v.z = pack_weight(j, prow, 16 * m + 4 * g + 2);
    v.w = pack_weight(j, prow, 16 * m + 4 * g + 3);
    *reinterpret_cast<float4 *>(dst) = v;
    return;
  }
  // [split][lane][8 bf16]: element e = physical channel 16 (2 mp + e / 4) + 4 g + e % 4
  unsigned hi16[8], mid16[8], lo16[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float w = pack_weight(j, prow, 16 * (2 * m + (e >> 2)) + 4 * g + (e & 3));
    hi16[e] = bf16_bits(w);
    const float r1 = w - bf16_value(hi16[e]);
    mid16[e] = bf16_bits(r1);
    lo16[e] = bf16_bits(r1 - bf16_value(mid16[e]));
  }
  auto quad = [](const unsigned (&b)[8]) {
    return make_uint4(b[0] | (b[1] << 16), b[2] | (b[3] << 16), b[4] | (b[5] << 16), b[6] | (b[7] << 16));
  };
  *reinterpret_cast<uint4 *>(dst) = quad(hi16);
  if (j.fmt == PACK_FMT_BF16X3) {
    *reinterpret_cast<uint4 *>(dst + 256) = quad(mid16);
    *reinterpret_cast<uint4 *>(dst + 512) = quad(lo16);
  }
}

}  // namespace pwclo

using namespace pwclo;

extern "C" void pwclo_pack_layers_kernel_wrapper(const PwcloPackJob *jobs, int njobs, int total_tiles) {
  PWCLO_REQUIRE(njobs >= 1 && total_tiles >= 2 * njobs, "pack_layers: njobs=%d, total_tiles=%d (every job has at least one "
                "operand tile and its bias tile)", njobs, total_tiles);
  PWCLO_REQUIRE(jobs != nullptr && (reinterpret_cast<uintptr_t>(jobs) & 7u) == 0u,
                "pack_layers: the job table must be a device pointer, 8-byte aligned%s", "");
  hipLaunchKernelGGL(pack_layers_kernel, dim3((unsigned)total_tiles), dim3(64), 0, current_stream(), jobs, njobs);
  check_launch("pack_layers");
}
