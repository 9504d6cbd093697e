// Row bodies of the raw-frame filters (KITTI and KITTI-360), shared by every kernel that reads raw sweeps: the stand-alone
// filters and sweep_filter_compact_kernel (warp.hip) and the training batch builder (train_batch.hip).  One definition, so
// all of them give the same coordinate bits and the same keep decision for a row.
#pragma once
#include <hip/hip_runtime.h>

namespace pwclo {

// Raw KITTI velodyne frame -> camera-frame cloud + keep mask (kitti_odometry_dataset.py:375-397 and
// filter_pcd :149-160): p' = Tr[:3,:4] . (x, y, z, 1) in fp64 like the reference's numpy matmul on the
// float64-promoted points, keep = not ground (y' <= 1.1) and |x'| < 30 and |z'| < 30 (strict, as
// the reference's `<` / `>`), coordinates stored as fp32.  One row; shared by kitti_transform_filter_kernel and
// sweep_filter_compact_kernel, so both give the same bits.
__device__ __forceinline__ bool kitti_row(const float4 p, const double *__restrict__ tr, float o3[3]) {
  const double x = p.x, y = p.y, z = p.z;
  double o[3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    o[r] = ((tr[r * 4 + 0] * x + tr[r * 4 + 1] * y) + tr[r * 4 + 2] * z) + tr[r * 4 + 3];
  const bool ground = o[1] > 1.1;
  const bool near = (o[0] < 30.0 && o[0] > -30.0) && (o[2] < 30.0 && o[2] > -30.0);
  o3[0] = (float)o[0];
  o3[1] = (float)o[1];
  o3[2] = (float)o[2];
  return !ground && near;
}

// KITTI-360 front end (slam/dataset/kitti_360_dataset_2.py:113-123): raw velodyne rows stay in the sensor
// frame; keep = not ground (z >= ground_z) and |x| < near and |y| < near, compared in fp32 as NumPy
// compares a float32 column with a Python scalar.  xyz = the first three columns.  One row, shared as kitti_row.
__device__ __forceinline__ bool kitti360_row(const float4 p, float ground_z, float near, float o3[3]) {
  const bool ground = p.z < ground_z;
  const bool close = (p.x < near && p.x > -near) && (p.y < near && p.y > -near);
  o3[0] = p.x;
  o3[1] = p.y;
  o3[2] = p.z;
  return !ground && close;
}

}  // namespace pwclo
