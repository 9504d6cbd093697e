// The keyframe gate of the knn refiner's local map: the arithmetic of one stream's decision, shared
// by the gate kernel of keyframe.hip and by anything on the device that wants the same numbers.  Everything is fp64 on
// se3.hpp's poses.
//
// The reference (slam/odometry/icp_odometry.py:361-381, __update_map) accumulates the motion since the last frame it put
// into the local map and inserts the new frame only when that motion exceeds a translation or a rotation threshold; below
// both, the map is only moved into the new frame.  Here the rotation is measured by its angle, not by the norm of its
// Euler angles: the two agree for a rotation about one axis and to second order otherwise, and the angle has no gimbal case.
#pragma once
#include <math.h>

#include "se3.hpp"

namespace pwclo {

constexpr double KEYFRAME_DEG = 57.29577951308232;        // 180 / pi

// |D[:3, 3]| of the accumulated motion
__device__ __forceinline__ double keyframe_translation(const Se3 &d) {
  return sqrt((d.m[3] * d.m[3] + d.m[7] * d.m[7]) + d.m[11] * d.m[11]);
}

// The rotation angle of D in degrees: atan2(s, c) with c = (trace - 1) / 2 and s = |axial vector of D - D^T| / 2, which
// keeps its precision at 0 and at 180 degrees where acos(c) alone loses half of it.
__device__ __forceinline__ double keyframe_angle_deg(const Se3 &d) {
  const double c = 0.5 * (((d.m[0] + d.m[5]) + d.m[10]) - 1.0);
  const double ax = d.m[9] - d.m[6], ay = d.m[2] - d.m[8], az = d.m[4] - d.m[1];      // R32 - R23, R13 - R31, R21 - R12
  const double s = 0.5 * sqrt((ax * ax + ay * ay) + az * az);
  return atan2(s, c) * KEYFRAME_DEG;
}

// Both comparisons are strict, as the reference's; NaN never inserts.
__device__ __forceinline__ bool keyframe_exceeds(const Se3 &d, double trans, double rot) {
  return keyframe_translation(d) > trans || keyframe_angle_deg(d) > rot;
}

}  // namespace pwclo
