// The keyframe gate of the knn registration refiner (gfx950).
//
// The reference does not put every frame into its local map (slam/odometry/icp_odometry.py:361-381): it accumulates the
// motion since the last inserted frame and inserts the new one only when that motion exceeds a threshold; otherwise the map
// is only moved into the new frame.  keyframe_gate_kernel takes that decision per stream, on the device, between the last
// solve and the push, so that one captured graph serves every decision: the gated push (icp.hip) reads kf_insert from
// device memory and the node sequence never changes.  The projective refiner has no gate.  No atomics, nothing sized
// from the data.
//
// State per stream: kf_delta (4x4 fp64, the motion since the stream's last inserted frame), kf_insert (this call's
// decision), kf_count (frames inserted since the map was emptied).  The rules, in this order:
//   idle (active[s] == 0)            nothing changes, kf_insert = 0
//   no live slot in the stream's map kf_insert = 1, kf_delta = I, kf_count = 1 (a first frame, a restart, a reset)
//   otherwise                        D = kf_delta . T[s]; insert iff |D[:3, 3]| > trans || angle(D) > rot (strict);
//                                    insert: kf_delta = I, kf_count += 1; no insert: kf_delta = D
#include "common.hpp"
#include "keyframe.hpp"

namespace pwclo {

constexpr int KEYFRAME_MAX_STREAMS = 1024;  // the refiner's MAX_STREAMS: one workgroup, one thread per stream
constexpr int KEYFRAME_MAX_SLOTS = 64;      // icp.hip: ICP_MAX_SLOTS

// T (S, 4, 4), live (S, M), active (S) or nullptr (every stream delivered a frame).  Every stream owns its words.
__global__ __launch_bounds__(KEYFRAME_MAX_STREAMS) void keyframe_gate_kernel(int S, int M, const double *__restrict__ T,
                                                                             const int *__restrict__ live,
                                                                             const int *__restrict__ active, double trans,
                                                                             double rot, double *__restrict__ kf_delta,
                                                                             int *__restrict__ kf_insert,
                                                                             int *__restrict__ kf_count) {
  const int s = threadIdx.x;
  if (s >= S) return;
  if (active != nullptr && active[s] == 0) {
    kf_insert[s] = 0;
    return;
  }
  bool any = false;
  for (int m = 0; m < M; ++m) any = any || live[s * M + m] != 0;
  double *delta = kf_delta + (size_t)s * 16;
  if (!any) {
    se3_store(delta, se3_identity());
    kf_insert[s] = 1;
    kf_count[s] = 1;
    return;
  }
  const Se3 d = se3_mul(se3_load(delta), se3_load(T + (size_t)s * 16));
  const bool ins = keyframe_exceeds(d, trans, rot);
  se3_store(delta, ins ? se3_identity() : d);
  kf_insert[s] = ins ? 1 : 0;
  if (ins) kf_count[s] += 1;
}

}  // namespace pwclo

using namespace pwclo;

extern "C" void keyframe_gate_kernel_wrapper(int S, int M, const double *T, const int *live, const int *active, double trans,
                                             double rot, double *kf_delta, int *kf_insert, int *kf_count) {
  if (S <= 0) return;
  PWCLO_REQUIRE(S <= KEYFRAME_MAX_STREAMS && M >= 1 && M <= KEYFRAME_MAX_SLOTS,
                "keyframe_gate: S=%d M=%d out of range (S <= %d, M <= %d)", S, M, KEYFRAME_MAX_STREAMS, KEYFRAME_MAX_SLOTS);
  PWCLO_REQUIRE(trans >= 0.0 && isfinite(trans) && rot >= 0.0 && isfinite(rot),
                "keyframe_gate: trans=%g and rot=%g must be finite and >= 0", trans, rot);
  PWCLO_REQUIRE(T != nullptr && live != nullptr && kf_delta != nullptr && kf_insert != nullptr && kf_count != nullptr,
                "keyframe_gate: every pointer but active is required%s", "");
  PWCLO_REQUIRE(aligned(T, 8) && aligned(kf_delta, 8),
                "keyframe_gate: fp64 arrays must be 8-byte aligned%s", "");
  hipLaunchKernelGGL(keyframe_gate_kernel, dim3(1), dim3(ceil_div(S, 64) * 64), 0, current_stream(), S, M, T, live, active,
                     trans, rot, kf_delta, kf_insert, kf_count);
  check_launch("keyframe_gate");
}
