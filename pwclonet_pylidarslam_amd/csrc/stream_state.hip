// The state machine of streaming odometry (gfx950).
//
// Every stream carries its own state on the device, driven by two masks loaded before every call -- active[s]: stream
// s delivered a frame; restart[s]: that frame starts a new sequence (lock step, section 11, is the case active = 1,
// restart = 0 for every stream):
//   idle   (!active)                          nothing moves, valid = 0
//   prime  (active && (restart || !have_prev))  rel[0,s] = abs[0,s] = I, count = 1, have_prev = 1, valid = 0
//   pair   (otherwise)                        k = count: rel[k,s] = quat2mat(row), abs[k,s] = abs[k-1,s] . rel[k,s],
//                                             count = k + 1, valid = 1
// stream_append_masked_kernel runs that machine, one thread per stream; stream_handover_masked_kernel then moves the
// new frame's state into the persistent previous frame for the active streams only, in ONE launch over a table of
// segments (it replaces one copy node per tensor); stream_record_refined_kernel keeps the refined trajectories of a
// masked registration beside the network's; stream_motion_from_refined_kernel hands a refined pose to the de-skew
// prior.  All four read their masks from device memory, so one captured graph serves priming, pairs and idling alike.
#include "common.hpp"
#include "se3.hpp"

namespace pwclo {

// pose: (S, 4, 7) fp32 contiguous, rows [tx ty tz qw qx qy qz] of levels 1..4; the level-1 row is appended.  Streams
// that are not `pair` get the identity pose (t = 0, q = (1, 0, 0, 0)) in all four rows: the caller never sees the pose
// of a pair that does not exist.  Every stream owns its own state words, so no thread reads what another writes.
__global__ __launch_bounds__(1024) void stream_append_masked_kernel(int S, int capacity, const int *__restrict__ active,
                                                                    const int *__restrict__ restart,
                                                                    float *__restrict__ pose, double *__restrict__ rel,
                                                                    double *__restrict__ abs_out,
                                                                    int *__restrict__ have_prev, int *__restrict__ count,
                                                                    int *__restrict__ valid, int *__restrict__ overflow) {
  const int i = threadIdx.x;
  if (i >= S) return;
  float *rows = pose + (size_t)i * 28;
  const bool act = active[i] != 0;
  const bool prime = act && (restart[i] != 0 || have_prev[i] == 0);
  if (act && !prime) {
    const int k = count[i];
    if (k < 1 || k >= capacity) {             // full (the host check keeps this unreachable): nothing is written
      *overflow = 1;
    } else {
      const size_t at = ((size_t)k * S + i) * 16;
      const Se3 t = pose_row_to_se3(rows);
      const Se3 a = se3_mul(se3_load(abs_out + at - (size_t)S * 16), t);
      se3_store(rel + at, t);
      se3_store(abs_out + at, a);
      count[i] = k + 1;
    }
    valid[i] = 1;
    return;
  }
  if (prime) {
    const Se3 id = se3_identity();
    se3_store(rel + (size_t)i * 16, id);
    se3_store(abs_out + (size_t)i * 16, id);
    count[i] = 1;
    have_prev[i] = 1;
  }
  valid[i] = 0;
#pragma unroll
  for (int l = 0; l < 4; ++l) {
#pragma unroll
    for (int j = 0; j < 7; ++j) rows[l * 7 + j] = j == 3 ? 1.0f : 0.0f;
  }
}

// After the masked registration of the call's frames (icp.hip): the refined trajectories beside rel /
// abs, at the row the append above just wrote.  active / valid / count: this call's words, count after the append; T (S, 4,
// 4): the refiner's poses.  A pair (active && valid) writes row k = count - 1: ref_rel[k,s] = T[s], ref_abs[k,s] =
// ref_abs[k-1,s] . T[s]; a stream that primed (active && !valid) writes the identity into row 0; an idle stream writes
// nothing.  The guard is the append's (a full stream wrote nothing there and writes nothing here); one thread per stream,
// every stream owns its rows.
__global__ __launch_bounds__(1024) void stream_record_refined_kernel(int S, int capacity, const int *__restrict__ active,
                                                                     const int *__restrict__ valid,
                                                                     const int *__restrict__ count,
                                                                     const double *__restrict__ T,
                                                                     double *__restrict__ ref_rel,
                                                                     double *__restrict__ ref_abs) {
  const int i = threadIdx.x;
  if (i >= S || active[i] == 0) return;
  if (valid[i] != 0) {
    const int k = count[i] - 1;
    if (k < 1 || k >= capacity) return;
    const size_t at = ((size_t)k * S + i) * 16;
    const Se3 t = se3_load(T + (size_t)i * 16);
    const Se3 a = se3_mul(se3_load(ref_abs + at - (size_t)S * 16), t);
    se3_store(ref_rel + at, t);
    se3_store(ref_abs + at, a);
    return;
  }
  const Se3 id = se3_identity();
  se3_store(ref_rel + (size_t)i * 16, id);
  se3_store(ref_abs + (size_t)i * 16, id);
}

// With refine=dict(..., feedback=True): the refined pose becomes the de-skew prior.  After the
// registration and before the record above, a pair (active && valid) overwrites its row of motion (S, 7) fp32 -- the rows
// stream_motion_handover_kernel (deskew.hip) writes, [tx ty tz qw qx qy qz] -- with the pose row of T[s]; every other stream's
// row (primed, idle, or written by the step's own handover) keeps its bits.  One thread per stream.
__global__ __launch_bounds__(1024) void stream_motion_from_refined_kernel(int S, const int *__restrict__ active,
                                                                          const int *__restrict__ valid,
                                                                          const double *__restrict__ T,
                                                                          float *__restrict__ motion) {
  const int i = threadIdx.x;
  if (i >= S || active[i] == 0 || valid[i] == 0) return;
  se3_to_pose_row(se3_load(T + (size_t)i * 16), motion + (size_t)i * 7);
}

// ---- masked handover -------------------------------------------------------------------------------------------------

constexpr int HANDOVER_MAX_SEGMENTS = 32;
constexpr int HANDOVER_THREADS = 256;
constexpr int HANDOVER_UNROLL = 4;                                                   // 16-byte loads in flight per lane
constexpr int HANDOVER_CHUNK = HANDOVER_THREADS * HANDOVER_UNROLL * 16;              // bytes per workgroup and round
constexpr int HANDOVER_MAX_CHUNKS = 64;       // grid.x cap: 64 x 16 KiB covers 1 MiB per round, larger segments loop

struct HandoverSegment {          // stream s: `bytes` bytes from src + s * src_stride to dst + s * dst_stride
  char *dst;
  const char *src;
  long long bytes, dst_stride, src_stride;
  int wide;                       // every address and the byte count are multiples of 16
};
struct HandoverTable {
  HandoverSegment seg[HANDOVER_MAX_SEGMENTS];
};

// grid (chunks, segments, S).  The mask word and the segment are the same for the whole workgroup (scalar loads, no
// divergence): an idle stream's workgroups return at once and touch no memory.  A workgroup round moves 16 KiB: in a
// whole round every lane issues four independent 16-byte loads into four registers and then its four stores (no LDS,
// no wait between the loads); the one partial round at a segment's end loads at clamped indices and guards its stores.
// Segments whose addresses, size or strides are not multiples of 16 go 4 bytes at a time, one load per lane in flight:
// that path serves the few small segments (a stream's length word) and is not tuned.
__global__ __launch_bounds__(HANDOVER_THREADS) void stream_handover_masked_kernel(HandoverTable table,
                                                                                  const int *__restrict__ active) {
  const int s = blockIdx.z;
  if (active[s] == 0) return;
  const HandoverSegment sg = table.seg[blockIdx.y];
  const long long bytes = sg.bytes;
  if ((long long)blockIdx.x * HANDOVER_CHUNK >= bytes) return;
  char *dst = sg.dst + (long long)s * sg.dst_stride;
  const char *src = sg.src + (long long)s * sg.src_stride;
  if (sg.wide) {
    const long long n = bytes >> 4;
    uint4 *d = reinterpret_cast<uint4 *>(dst);
    const uint4 *g = reinterpret_cast<const uint4 *>(src);
    const long long step = (long long)gridDim.x * (HANDOVER_THREADS * HANDOVER_UNROLL);
    constexpr int ROUND = HANDOVER_THREADS * HANDOVER_UNROLL;
    for (long long base = (long long)blockIdx.x * ROUND; base < n; base += step) {
      const long long e0 = base + threadIdx.x;
      // four named registers, not an array: an array written under a branch is moved to LDS by the compiler, which
      // puts a wait and an LDS round trip behind every load
      static_assert(HANDOVER_UNROLL == 4, "the rounds below are written out for four loads per lane");
      const long long e1 = e0 + HANDOVER_THREADS, e2 = e0 + 2 * HANDOVER_THREADS, e3 = e0 + 3 * HANDOVER_THREADS;
      if (base + ROUND <= n) {                // a whole round (the same for every lane): no guards
        const uint4 v0 = g[e0], v1 = g[e1], v2 = g[e2], v3 = g[e3];
        d[e0] = v0;
        d[e1] = v1;
        d[e2] = v2;
        d[e3] = v3;
      } else {                                // the segment's tail: loads at a clamped index, guarded stores
        const long long last = n - 1;
        const uint4 v0 = g[e0 < n ? e0 : last], v1 = g[e1 < n ? e1 : last], v2 = g[e2 < n ? e2 : last],
                    v3 = g[e3 < n ? e3 : last];
        if (e0 < n) d[e0] = v0;
        if (e1 < n) d[e1] = v1;
        if (e2 < n) d[e2] = v2;
        if (e3 < n) d[e3] = v3;
      }
    }
  } else {
    const long long n = bytes >> 2;
    unsigned *d = reinterpret_cast<unsigned *>(dst);
    const unsigned *g = reinterpret_cast<const unsigned *>(src);
    const long long per = HANDOVER_CHUNK / 4;                   // the same 16 KiB per workgroup round
    const long long step = (long long)gridDim.x * per;
    for (long long base = (long long)blockIdx.x * per; base < n; base += step) {
      const long long end = base + per < n ? base + per : n;
      for (long long e = base + threadIdx.x; e < end; e += HANDOVER_THREADS) d[e] = g[e];
    }
  }
}

}  // namespace pwclo

using namespace pwclo;

extern "C" void stream_append_masked_kernel_wrapper(int S, int capacity, const int *active, const int *restart, float *pose,
                                                    double *rel, double *abs_out, int *have_prev, int *count, int *valid,
                                                    int *overflow) {
  PWCLO_REQUIRE(S >= 1 && S <= 1024, "stream_append_masked: S=%d streams outside one workgroup [1, 1024]", S);
  PWCLO_REQUIRE(capacity >= 1, "stream_append_masked: capacity=%d must be >= 1", capacity);
  PWCLO_REQUIRE(active && restart && pose && rel && abs_out && have_prev && count && valid && overflow,
                "stream_append_masked: a null argument");
  hipLaunchKernelGGL(stream_append_masked_kernel, dim3(1), dim3(ceil_div(S, 64) * 64), 0, current_stream(), S, capacity,
                     active, restart, pose, rel, abs_out, have_prev, count, valid, overflow);
  check_launch("stream_append_masked");
}

extern "C" void stream_record_refined_kernel_wrapper(int S, int capacity, const int *active, const int *valid,
                                                     const int *count, const double *T, double *ref_rel, double *ref_abs) {
  PWCLO_REQUIRE(S >= 1 && S <= 1024, "stream_record_refined: S=%d streams outside one workgroup [1, 1024]", S);
  PWCLO_REQUIRE(capacity >= 1, "stream_record_refined: capacity=%d must be >= 1", capacity);
  PWCLO_REQUIRE(active && valid && count && T && ref_rel && ref_abs, "stream_record_refined: a null argument");
  PWCLO_REQUIRE(((reinterpret_cast<uintptr_t>(T) | reinterpret_cast<uintptr_t>(ref_rel) |
                  reinterpret_cast<uintptr_t>(ref_abs)) & 7) == 0,
                "stream_record_refined: fp64 arrays must be 8-byte aligned");
  hipLaunchKernelGGL(stream_record_refined_kernel, dim3(1), dim3(ceil_div(S, 64) * 64), 0, current_stream(), S, capacity,
                     active, valid, count, T, ref_rel, ref_abs);
  check_launch("stream_record_refined");
}

extern "C" void stream_motion_from_refined_kernel_wrapper(int S, const int *active, const int *valid, const double *T,
                                                          float *motion) {
  PWCLO_REQUIRE(S >= 1 && S <= 1024, "stream_motion_from_refined: S=%d streams outside one workgroup [1, 1024]", S);
  PWCLO_REQUIRE(active && valid && T && motion, "stream_motion_from_refined: a null argument");
  PWCLO_REQUIRE((reinterpret_cast<uintptr_t>(T) & 7) == 0, "stream_motion_from_refined: T must be 8-byte aligned");
  hipLaunchKernelGGL(stream_motion_from_refined_kernel, dim3(1), dim3(ceil_div(S, 64) * 64), 0, current_stream(), S, active,
                     valid, T, motion);
  check_launch("stream_motion_from_refined");
}

extern "C" int stream_handover_max_segments(void) { return HANDOVER_MAX_SEGMENTS; }

extern "C" void stream_handover_masked_kernel_wrapper(int nseg, void *const *dst, const void *const *src,
                                                      const long long *bytes, const long long *dst_stride,
                                                      const long long *src_stride, int S, const int *active) {
  if (nseg == 0) return;
  PWCLO_REQUIRE(nseg >= 1 && nseg <= HANDOVER_MAX_SEGMENTS, "stream_handover_masked: %d segments outside [1, %d]", nseg,
                HANDOVER_MAX_SEGMENTS);
  PWCLO_REQUIRE(S >= 1 && S <= 65535, "stream_handover_masked: S=%d streams outside the grid limit [1, 65535]", S);
  PWCLO_REQUIRE(dst && src && bytes && active, "stream_handover_masked: a null argument");
  HandoverTable table;
  long long longest = 0;
  for (int i = 0; i < HANDOVER_MAX_SEGMENTS; ++i) {
    HandoverSegment &sg = table.seg[i];
    if (i >= nseg) {
      sg = HandoverSegment{nullptr, nullptr, 0, 0, 0, 0};
      continue;
    }
    sg.dst = static_cast<char *>(dst[i]);
    sg.src = static_cast<const char *>(src[i]);
    sg.bytes = bytes[i];
    sg.dst_stride = dst_stride ? dst_stride[i] : bytes[i];
    sg.src_stride = src_stride ? src_stride[i] : bytes[i];
    const unsigned long long every = (unsigned long long)(uintptr_t)sg.dst | (unsigned long long)(uintptr_t)sg.src |
                                     (unsigned long long)sg.bytes | (unsigned long long)sg.dst_stride |
                                     (unsigned long long)sg.src_stride;
    PWCLO_REQUIRE(sg.dst && sg.src && sg.bytes >= 0 && sg.dst_stride >= sg.bytes && sg.src_stride >= sg.bytes,
                  "stream_handover_masked: segment %d has a null pointer or a stride below its %lld bytes", i, sg.bytes);
    PWCLO_REQUIRE((every & 3) == 0, "stream_handover_masked: segment %d is not 4-byte aligned in address, size or stride", i);
    sg.wide = (every & 15) == 0;
    if (sg.bytes > longest) longest = sg.bytes;
  }
  if (longest == 0) return;
  long long chunks = (longest + HANDOVER_CHUNK - 1) / HANDOVER_CHUNK;
  if (chunks > HANDOVER_MAX_CHUNKS) chunks = HANDOVER_MAX_CHUNKS;
  hipLaunchKernelGGL(stream_handover_masked_kernel, dim3((unsigned)chunks, nseg, S), dim3(HANDOVER_THREADS), 0,
                     current_stream(), table, active);
  check_launch("stream_handover_masked");
}
