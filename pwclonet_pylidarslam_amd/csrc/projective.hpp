// Arithmetic of the projective frame-to-model registration on spherical vertex maps, shared by the
// kernels of projective.hip and by host code that wants the same numbers (the pattern of icp.hpp): one definition of a
// point's pixel, of a z-buffer key and of a pixel's normal.  Poses and their inverses are se3.hpp's.
//
// The reference's ICPFrameToModel over a ProjectiveLocalMap (slam/odometry/local_map.py:84-240) projects every sweep to a
// spherical image (slam/common/projection.py:20-82, 340-436), takes normals from box-filtered moments of that image
// (slam/common/geometry.py:248-303) and associates a point with whatever sits at its own pixel (geometry.py:405-447).
// The pixel is computed in fp32 in the reference's order of operations; the moments are fp64 sums of the fp32 vertices.
#pragma once
#include <math.h>
#include <stdint.h>

#include "common.hpp"
#include "icp.hpp"

namespace pwclo {

// An image: height, width, and the two fp32 constants of the row formula, |down_fov| and |up_fov| + |down_fov| in radians
// (computed in fp64 from the degrees and rounded once, as the reference's Python scalars are when they meet an fp32 tensor).
struct ProjImage {
  int H, W;
  float down, fov;
};

constexpr unsigned long long PROJ_EMPTY_KEY = ~0ull;
constexpr float PROJ_PI = 3.14159265358979323846f;
constexpr float PROJ_DET_EPS = 1e-6f;       // compute_normal_map's bound on |det C|, held in fp32 there

ICP_HD ProjImage proj_image(int H, int W, double up_fov_deg, double down_fov_deg) {
  const double up = up_fov_deg / 180.0 * M_PI, down = down_fov_deg / 180.0 * M_PI;
  ProjImage im;
  im.H = H; im.W = W;
  im.down = (float)fabs(down);
  im.fov = (float)(fabs(down) + fabs(up));
  return im;
}

// The pixel of the point (x, y, z): false when the point has no pixel (r = 0 or not finite, or the rounded row / column is
// outside the image; NaN fails every comparison).  r: the range, row / col: the pixel, rounded half to even.
ICP_HD bool proj_pixel(const ProjImage &im, float x, float y, float z, float *r_out, int *row_out, int *col_out) {
  const float r = sqrtf((x * x + y * y) + z * z);
  *r_out = r;
  if (!(r > 0.0f) || !(r <= 3.402823466e+38f)) return false;
  const float theta = -atan2f(y, x);
  const float phi = asinf(z / r);
  const float col = (0.5f * (theta / PROJ_PI + 1.0f)) * (float)im.W;
  const float row = (1.0f - (phi + im.down) / im.fov) * (float)im.H;
  const float rr = rintf(row), rc = rintf(col);
  if (!(rr >= 0.0f && rr <= (float)(im.H - 1) && rc >= 0.0f && rc <= (float)(im.W - 1))) return false;
  *row_out = (int)rr;
  *col_out = (int)rc;
  return true;
}

// r > 0, so its bits order as the value does: the smallest key is the nearest point, the lowest index among equal ranges.
ICP_HD unsigned long long proj_key(float r, unsigned int index) {
#if defined(__HIP_DEVICE_COMPILE__)
  const unsigned int bits = __float_as_uint(r);
#else
  unsigned int bits;
  memcpy(&bits, &r, 4);
#endif
  return ((unsigned long long)bits << 32) | (unsigned long long)index;
}

// The normal of a pixel from the moments of its window about the sensor: m = sum p (3), c = sum p p^T ([xx xy xz yy yz zz]).
// n = C^-1 m by the adjugate over the determinant, normalised and rounded once to fp32; zero where |fp32(det)| <= 1e-6 or
// |n| = 0 (NaN gives zero too).
ICP_HD void proj_normal(const double m[3], const double c[6], float out[3]) {
  const double xx = c[0], xy = c[1], xz = c[2], yy = c[3], yz = c[4], zz = c[5];
  const double a00 = yy * zz - yz * yz, a01 = xz * yz - xy * zz, a02 = xy * yz - xz * yy;
  const double a11 = xx * zz - xz * xz, a12 = xy * xz - xx * yz, a22 = xx * yy - xy * xy;
  const double det = (xx * a00 + xy * a01) + xz * a02;
  out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f;
  if (!(fabsf((float)det) > PROJ_DET_EPS)) return;
  const double nx = ((a00 * m[0] + a01 * m[1]) + a02 * m[2]) / det;
  const double ny = ((a01 * m[0] + a11 * m[1]) + a12 * m[2]) / det;
  const double nz = ((a02 * m[0] + a12 * m[1]) + a22 * m[2]) / det;
  const double len = sqrt((nx * nx + ny * ny) + nz * nz);
  if (!(len > 0.0) || !(len <= 1.7976931348623157e308)) return;
  out[0] = (float)(nx / len); out[1] = (float)(ny / len); out[2] = (float)(nz / len);
}

}  // namespace pwclo
