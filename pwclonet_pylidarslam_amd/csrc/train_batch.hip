// Training batches from raw LiDAR pairs (batches.TrainBatchBuilder).  Replaces the host NumPy of the
// reference's training __getitem__ (slam/dataset/kitti_odometry_dataset.py:375-463, kitti_360_dataset_2.py:113-135,
// 174-272): cut both frames to the shorter one, filter, a random choice of npoints survivors, a random rigid augmentation
// of frame 2 and the ground truth composed with it.  Two launches per batch:
//   train_batch_pose_kernel    one workgroup; per pair: six clipped normals, T_trans, T_gt, the quaternion and gt (fp64),
//                              and the step counter's hand-over (state[2] = state[1]++), after every thread has read it;
//   train_batch_sample_kernel  one 1024-thread workgroup per cloud: count, radix select of the npoints smallest random
//                              keys, bitonic sort in LDS, write phase.
// Random numbers are Philox4x32-10 words addressed by (index, cloud or pair, step, purpose) under the 64-bit seed: every
// word can be recomputed anywhere, nothing is stored, and a batch is a function of (seed, step, inputs) alone.  Lengths,
// calibration, seed and step live in device memory, so one captured graph of the two launches serves every length and step.
#include <float.h>
#include <stdint.h>

#include "common.hpp"
#include "philox.hpp"
#include "rows.hpp"

namespace pwclo {

// c = a . b for 3x3 row-major matrices, every entry summed left to right.
__device__ __forceinline__ void mat3_mul(const double a[9], const double b[9], double c[9]) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k)
      c[r * 3 + k] = (a[r * 3 + 0] * b[0 * 3 + k] + a[r * 3 + 1] * b[1 * 3 + k]) + a[r * 3 + 2] * b[2 * 3 + k];
}

// Pose side of a batch, one thread per pair.  mode 0: no augmentation (T_trans = I, T_gt = T_diff); 1: draw the six
// parameters; 2: take them from aug_params as the caller left them.  state = {seed, next step, step in flight}.
__global__ __launch_bounds__(256) void train_batch_pose_kernel(int B, int kitti, int mode, long long *__restrict__ state,
                                                               const double *__restrict__ t_diff,
                                                               float *__restrict__ aug_params, double *__restrict__ t_trans,
                                                               double *__restrict__ t_gt, float *__restrict__ gt) {
  const unsigned long long seed = (unsigned long long)state[0];
  const long long step64 = state[1];
  __syncthreads();                                       // every thread holds the step before thread 0 moves it on
  if (threadIdx.x == 0) {
    state[2] = step64;
    state[1] = step64 + 1;
  }
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32), step = (unsigned)step64;
  const double scale[6] = {0.01, 0.05, 0.01, 0.1, 0.05, 0.5}, clip[6] = {0.02, 0.1, 0.02, 0.2, 0.15, 1.0};
  for (int b = threadIdx.x; b < B; b += 256) {
    float prm[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      if (mode == 1) {
        unsigned w[4];
        philox4x32_10((unsigned)j, (unsigned)b, step, TB_AUGMENT, k0, k1, w);
        const double u1 = ((double)w[0] + 0.5) * 0x1p-32, u2 = ((double)w[1] + 0.5) * 0x1p-32;
        const double z = sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925 * u2);
        const double v = scale[j] * z;
        prm[j] = (float)fmin(fmax(v, -clip[j]), clip[j]);
      } else {
        prm[j] = mode == 2 ? aug_params[b * 6 + j] : 0.0f;
      }
      aug_params[b * 6 + j] = prm[j];
    }
    double Rd[9], td[3], Rg[9], tg[3], T[12];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int k = 0; k < 3; ++k) Rd[r * 3 + k] = t_diff[b * 12 + r * 4 + k];
      td[r] = t_diff[b * 12 + r * 4 + 3];
    }
    if (mode == 0) {
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { T[r * 4 + k] = r == k ? 1.0 : 0.0; Rg[r * 3 + k] = Rd[r * 3 + k]; }
        T[r * 4 + 3] = 0.0;
        tg[r] = td[r];
      }
    } else {
      const double ax = (double)prm[0] * 3.14159265358979323846 / 4.0, ay = (double)prm[1] * 3.14159265358979323846 / 4.0,
                   az = (double)prm[2] * 3.14159265358979323846 / 4.0;
      const double cx = cos(ax), sx = sin(ax), cy = cos(ay), sy = sin(ay), cz = cos(az), sz = sin(az);
      const double Rx[9] = {1, 0, 0, 0, cx, -sx, 0, sx, cx}, Ry[9] = {cy, 0, sy, 0, 1, 0, -sy, 0, cy},
                   Rz[9] = {cz, -sz, 0, sz, cz, 0, 0, 0, 1};
      double Rxy[9], R[9];
      mat3_mul(Rx, Ry, Rxy);
      mat3_mul(Rxy, Rz, R);
      const double t[3] = {(double)prm[3], (double)prm[4], (double)prm[5]};
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 3; ++k) T[r * 4 + k] = R[r * 3 + k];
        T[r * 4 + 3] = t[r];
      }
      if (kitti) {                                       // T_gt = T_diff . inv(T_trans), inv = [R^T | -R^T t]
        double Ri[9], ti[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
          for (int k = 0; k < 3; ++k) Ri[r * 3 + k] = R[k * 3 + r];
          ti[r] = -((R[0 * 3 + r] * t[0] + R[1 * 3 + r] * t[1]) + R[2 * 3 + r] * t[2]);
        }
        mat3_mul(Rd, Ri, Rg);
#pragma unroll
        for (int r = 0; r < 3; ++r)
          tg[r] = ((Rd[r * 3 + 0] * ti[0] + Rd[r * 3 + 1] * ti[1]) + Rd[r * 3 + 2] * ti[2]) + td[r];
      } else {                                           // T_gt = T_trans . T_diff
        mat3_mul(R, Rd, Rg);
#pragma unroll
        for (int r = 0; r < 3; ++r)
          tg[r] = ((R[r * 3 + 0] * td[0] + R[r * 3 + 1] * td[1]) + R[r * 3 + 2] * td[2]) + t[r];
      }
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) t_trans[b * 12 + i] = T[i];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int k = 0; k < 3; ++k) t_gt[b * 16 + r * 4 + k] = Rg[r * 3 + k];
      t_gt[b * 16 + r * 4 + 3] = tg[r];
      t_gt[b * 16 + 12 + r] = 0.0;
    }
    t_gt[b * 16 + 15] = 1.0;
    double q[4];                                         // (w, x, y, z)
    if (kitti) {                                         // mat2euler ("zyx") then euler2quat, as the dataset does
      const double c = sqrt(Rg[8] * Rg[8] + Rg[5] * Rg[5]);
      double ez, ey, ex;
      if (c > DBL_EPSILON * 4.0) {
        ez = atan2(-Rg[1], Rg[0]);
        ey = atan2(Rg[2], c);
        ex = atan2(-Rg[5], Rg[8]);
      } else {
        ez = atan2(Rg[3], Rg[4]);
        ey = atan2(Rg[2], c);
        ex = 0.0;
      }
      const double hz = ez / 2.0, hy = ey / 2.0, hx = ex / 2.0;
      const double cz = cos(hz), sz = sin(hz), cy = cos(hy), sy = sin(hy), cx = cos(hx), sx = sin(hx);
      q[0] = cx * cy * cz - sx * sy * sz;
      q[1] = cx * sy * sz + cy * cz * sx;
      q[2] = cx * cz * sy - sx * cy * sz;
      q[3] = cx * cy * sz + sx * cz * sy;
    } else {                                             // largest of (m00, m11, m22, trace) picks the branch, then normalise
      const double tr = (Rg[0] + Rg[4]) + Rg[8];
      int ch = 0;
      double best = Rg[0];
      if (Rg[4] > best) { best = Rg[4]; ch = 1; }
      if (Rg[8] > best) { best = Rg[8]; ch = 2; }
      if (tr > best) ch = 3;
      double v[4];                                       // (x, y, z, w)
      if (ch != 3) {
        const int i = ch, j = (i + 1) % 3, k = (j + 1) % 3;
        v[i] = 1.0 - tr + 2.0 * Rg[i * 3 + i];
        v[j] = Rg[j * 3 + i] + Rg[i * 3 + j];
        v[k] = Rg[k * 3 + i] + Rg[i * 3 + k];
        v[3] = Rg[k * 3 + j] - Rg[j * 3 + k];
      } else {
        v[0] = Rg[2 * 3 + 1] - Rg[1 * 3 + 2];
        v[1] = Rg[0 * 3 + 2] - Rg[2 * 3 + 0];
        v[2] = Rg[1 * 3 + 0] - Rg[0 * 3 + 1];
        v[3] = 1.0 + tr;
      }
      const double nrm = sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3]);
      q[0] = v[3] / nrm; q[1] = v[0] / nrm; q[2] = v[1] / nrm; q[3] = v[2] / nrm;
    }
    gt[b * 7 + 0] = (float)tg[0]; gt[b * 7 + 1] = (float)tg[1]; gt[b * 7 + 2] = (float)tg[2];
    gt[b * 7 + 3] = (float)q[0]; gt[b * 7 + 4] = (float)q[1]; gt[b * 7 + 5] = (float)q[2]; gt[b * 7 + 6] = (float)q[3];
  }
}

// One workgroup per cloud c = 2 * pair + frame (frame 0 = pc1, 1 = pc2).  keys: P 64-bit LDS slots, P = the power of two
// >= npoints (dynamic LDS).  Wave w owns a contiguous range of rows and walks it 64 rows at a time, as
// sweep_filter_compact_kernel does, so ballot / popcount slots are in frame order.  Every pass recomputes the row body and
// the row's Philox word: nothing per row is stored.
template <bool KITTI>
__global__ __launch_bounds__(1024) void train_batch_sample_kernel(int R, int npoints, int P, const int *__restrict__ lengths,
                                                                  const float *__restrict__ sweeps,
                                                                  const double *__restrict__ tr, float ground_z, float near,
                                                                  const long long *__restrict__ state,
                                                                  const double *__restrict__ t_trans, int augmented,
                                                                  float *__restrict__ xyz_f1, float *__restrict__ xyz_f2,
                                                                  int *__restrict__ indices, int *__restrict__ counts) {
  extern __shared__ unsigned long long tb_keys[];
  __shared__ int wave_total[16];
  __shared__ unsigned hist[256];
  __shared__ unsigned collected;
  const int c = blockIdx.x, b = c >> 1, f = c & 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = min(min(max(lengths[2 * b], 0), R), min(max(lengths[2 * b + 1], 0), R));
  const unsigned long long seed = (unsigned long long)state[0];
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32), step = (unsigned)state[2];
  const int per_wave = ((n + 15) / 16 + 63) / 64 * 64;          // multiple of 64: steps never straddle two waves' ranges
  const int i0 = wave * per_wave, i1 = min(n, i0 + per_wave);
  const float *sf = sweeps + (size_t)c * R * 4;
  const double *ts = KITTI ? tr + (size_t)b * 12 : nullptr;
  auto row = [&](int i, float o[3]) {
    const float4 p = *reinterpret_cast<const float4 *>(sf + (size_t)i * 4);
    return KITTI ? kitti_row(p, ts, o) : kitti360_row(p, ground_z, near, o);
  };
  auto word = [&](int i) { return philox_word((unsigned)i, (unsigned)c, step, TB_SELECT, k0, k1); };
  // wave totals of a per-wave count -> (sum of the waves before this one, sum of all)
  auto wave_scan = [&](int total, int &base, int &all) {
    __syncthreads();
    if (lane == 0) wave_total[wave] = total;
    __syncthreads();
    base = 0; all = 0;
    for (int w = 0; w < 16; ++w) {
      const int t = wave_total[w];
      if (w < wave) base += t;
      all += t;
    }
  };

  int total = 0;
  for (int i = i0 + lane; i - lane < i1; i += 64) {
    float o[3];
    total += __popcll(__ballot(i < i1 && row(i, o)));
  }
  int base, count;
  wave_scan(total, base, count);

  if (count >= npoints) {
    // ---- radix select of the npoints-th smallest word, most significant digit first -------------------------------
    unsigned prefix = 0u, mask = 0u, need = (unsigned)npoints, ties = 0u;
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (tid < 256) hist[tid] = 0u;
      __syncthreads();
      for (int i = i0 + lane; i < i1; i += 64) {
        float o[3];
        if (row(i, o)) {
          const unsigned w = word(i);
          if ((w & mask) == prefix) atomicAdd(&hist[(w >> shift) & 255u], 1u);
        }
      }
      __syncthreads();
      unsigned cum = 0u, d = 255u;
      for (unsigned k = 0; k < 256u; ++k) {              // the same walk in every thread (LDS broadcast reads)
        const unsigned h = hist[k];
        if (cum + h >= need) { d = k; ties = h; break; }
        cum += h;
      }
      need -= cum;
      prefix |= d << shift;
      mask |= 255u << shift;
      __syncthreads();
    }
    // `need` of the `ties` survivors whose word equals prefix are selected, lowest rows first (the key's low half)
    int tie_base = 0;
    if (ties != need) {
      int t = 0;
      for (int i = i0 + lane; i - lane < i1; i += 64) {
        float o[3];
        t += __popcll(__ballot(i < i1 && row(i, o) && word(i) == prefix));
      }
      int all;
      wave_scan(t, tie_base, all);
    }
    if (tid == 0) collected = 0u;
    __syncthreads();
    for (int i = i0 + lane; i - lane < i1; i += 64) {
      float o[3];
      const bool surv = i < i1 && row(i, o);
      const unsigned w = surv ? word(i) : 0u;
      bool sel = surv && w < prefix;
      const bool tie = surv && w == prefix;
      if (ties == need) {
        sel = sel || tie;
      } else {
        const unsigned long long tm = __ballot(tie);
        sel = sel || (tie && tie_base + mbcnt64(tm) < (int)need);
        tie_base += __popcll(tm);
      }
      const unsigned long long m = __ballot(sel);
      unsigned slot0 = 0u;
      if (lane == 0 && m != 0ull) slot0 = atomicAdd(&collected, (unsigned)__popcll(m));
      slot0 = (unsigned)__builtin_amdgcn_readfirstlane((int)slot0);
      const unsigned slot = slot0 + (unsigned)mbcnt64(m);
      if (sel && slot < (unsigned)P) tb_keys[slot] = ((unsigned long long)w << 32) | (unsigned)i;
    }
    for (int j = npoints + tid; j < P; j += 1024) tb_keys[j] = ~0ull;
    __syncthreads();
    // ---- bitonic sort of the P keys, ascending --------------------------------------------------------------------
    for (int k = 2; k <= P; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < P / 2; t += 1024) {
          const int lo = 2 * t - (t & (j - 1)), hi = lo + j;
          const unsigned long long a = tb_keys[lo], z = tb_keys[hi];
          if ((a > z) == ((lo & k) == 0)) { tb_keys[lo] = z; tb_keys[hi] = a; }
        }
        __syncthreads();
      }
    }
  } else if (count > 0) {
    // ---- all survivors in frame order; the rest is drawn with replacement from that list below ---------------------
    for (int i = i0 + lane; i - lane < i1; i += 64) {
      float o[3];
      const bool k = i < i1 && row(i, o);
      const unsigned long long m = __ballot(k);
      const int p = base + mbcnt64(m);
      if (k && p < P) tb_keys[p] = (unsigned)i;
      base += __popcll(m);
    }
    __syncthreads();
  }

  // ---- write phase: point j of the cloud <- raw row r_j, channel-major -------------------------------------------------
  const bool second = KITTI ? f == 0 : f == 1;             // KITTI hands the pair over swapped: xyz_f1 = augmented pc2
  float *dst = (second ? xyz_f2 : xyz_f1) + (size_t)b * 3 * npoints;
  const bool aug = augmented != 0 && f == 1;
  double T[12];
  if (aug)
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = t_trans[(size_t)b * 12 + i];
  for (int j = tid; j < npoints; j += 1024) {
    int r;
    if (count >= npoints || j < count) {
      r = (int)(unsigned)tb_keys[j];
    } else if (count > 0) {
      const unsigned w = philox_word((unsigned)(j - count), (unsigned)c, step, TB_REPLACE, k0, k1);
      r = (int)(unsigned)tb_keys[(unsigned)(((unsigned long long)w * (unsigned)count) >> 32)];
    } else if (n > 0) {
      const unsigned w = philox_word((unsigned)j, (unsigned)c, step, TB_REPLACE, k0, k1);
      r = (int)(unsigned)(((unsigned long long)w * (unsigned)n) >> 32);
    } else {
      r = -1;                                              // no rows at all (a device length <= 0): a zero point
    }
    float o[3] = {0.0f, 0.0f, 0.0f};
    if (r >= 0 && r < n) {
      row(r, o);
      if (aug) {
        const double x = o[0], y = o[1], z = o[2];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) o[ch] = (float)(((T[ch * 4 + 0] * x + T[ch * 4 + 1] * y) + T[ch * 4 + 2] * z) + T[ch * 4 + 3]);
      }
    }
    dst[j] = o[0];
    dst[npoints + j] = o[1];
    dst[2 * npoints + j] = o[2];
    indices[(size_t)c * npoints + j] = r;
  }
  if (tid == 0) counts[c] = count;
}

}  // namespace pwclo

using namespace pwclo;

extern "C" void train_batch_pose_kernel_wrapper(int B, int dataset, int mode, long long *state, const double *t_diff,
                                                float *aug_params, double *t_trans, double *t_gt, float *gt) {
  if (B <= 0) return;
  PWCLO_REQUIRE(dataset == 0 || dataset == 1, "train_batch_pose: dataset=%d (0 = KITTI, 1 = KITTI-360)", dataset);
  PWCLO_REQUIRE(mode >= 0 && mode <= 2, "train_batch_pose: mode=%d (0 = no augmentation, 1 = drawn, 2 = given)", mode);
  PWCLO_REQUIRE(state != nullptr && t_diff != nullptr && aug_params != nullptr && t_trans != nullptr && t_gt != nullptr &&
                gt != nullptr, "train_batch_pose: every pointer is required%s", "");
  hipLaunchKernelGGL(train_batch_pose_kernel, dim3(1), dim3(256), 0, current_stream(), B, dataset == 0 ? 1 : 0, mode, state,
                     t_diff, aug_params, t_trans, t_gt, gt);
  check_launch("train_batch_pose");
}

extern "C" void train_batch_sample_kernel_wrapper(int B, int R, int npoints, int dataset, const int *lengths,
                                                  const float *sweeps, const double *tr, float ground_z, float near,
                                                  const long long *state, const double *t_trans, int augmented,
                                                  float *xyz_f1, float *xyz_f2, int *indices, int *counts) {
  if (B <= 0) return;
  PWCLO_REQUIRE(R > 0 && (long long)R * 4 < (1ll << 31), "train_batch_sample: R=%d out of range", R);
  PWCLO_REQUIRE(npoints >= 1 && npoints <= 8192, "train_batch_sample: npoints=%d outside [1, 8192] (the selection lives in LDS)",
                npoints);
  PWCLO_REQUIRE(dataset == 0 || dataset == 1, "train_batch_sample: dataset=%d (0 = KITTI, 1 = KITTI-360)", dataset);
  PWCLO_REQUIRE(lengths != nullptr && sweeps != nullptr && state != nullptr && xyz_f1 != nullptr && xyz_f2 != nullptr &&
                indices != nullptr && counts != nullptr && (dataset == 1 || tr != nullptr) &&
                (augmented == 0 || t_trans != nullptr),
                "train_batch_sample: lengths, sweeps, state, outputs (tr for KITTI, t_trans when augmented) are required%s", "");
  PWCLO_REQUIRE((reinterpret_cast<uintptr_t>(sweeps) & 15) == 0, "train_batch_sample: sweeps must be 16-byte aligned%s", "");
  int P = 2;
  while (P < npoints) P *= 2;
  const size_t lds = (size_t)P * sizeof(unsigned long long);
  static bool attr = false;                              // once (the first call is made outside any capture): P * 8 = 64 KiB
  if (!attr) {                                           // at npoints 8192, plus the static histogram: above the 64 KiB default
    (void)hipFuncSetAttribute((const void *)train_batch_sample_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 72 * 1024);
    (void)hipFuncSetAttribute((const void *)train_batch_sample_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 72 * 1024);
    attr = true;
  }
  if (dataset == 0)
    hipLaunchKernelGGL(train_batch_sample_kernel<true>, dim3(2 * B), dim3(1024), lds, current_stream(), R, npoints, P, lengths,
                       sweeps, tr, ground_z, near, state, t_trans, augmented, xyz_f1, xyz_f2, indices, counts);
  else
    hipLaunchKernelGGL(train_batch_sample_kernel<false>, dim3(2 * B), dim3(1024), lds, current_stream(), R, npoints, P, lengths,
                       sweeps, tr, ground_z, near, state, t_trans, augmented, xyz_f1, xyz_f2, indices, counts);
  check_launch("train_batch_sample");
}
