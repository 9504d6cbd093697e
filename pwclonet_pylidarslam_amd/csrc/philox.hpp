// Counter-based random words shared by every kernel that draws them: the training batch builder (train_batch.hip) and the
// training pose head's dropout masks (pose_head_train.hip).  One definition, so a word addressed by
// (index, unit, step, purpose) under a seed has the same bits wherever it is recomputed.
#pragma once
#include <hip/hip_runtime.h>

namespace pwclo {

// purpose words of the counter (c3): one per use, so no two uses ever share a word
constexpr unsigned TB_SELECT = 0u;    // train_batch: selection keys
constexpr unsigned TB_REPLACE = 1u;   // train_batch: draws with replacement
constexpr unsigned TB_AUGMENT = 2u;   // train_batch: augmentation normals
constexpr unsigned PH_DROPOUT = 3u;   // pose_head_train: keep bits

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), counter (c0..c3), key (k0, k1).
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ unsigned philox_word(unsigned index, unsigned unit, unsigned step, unsigned purpose, unsigned k0,
                                                unsigned k1) {
  unsigned o[4];
  philox4x32_10(index, unit, step, purpose, k0, k1, o);
  return o[0];
}

}  // namespace pwclo
