// Projective frame-to-model registration on spherical vertex maps (gfx950).
//
// The reference's default odometry, ICPFrameToModel over a ProjectiveLocalMap (slam/odometry/local_map.py:84-240): every
// sweep becomes a spherical vertex map, normals come from box-filtered moments of that image, the last frames are
// re-projected into the newest frame's view, and a point's neighbour is whatever sits at its own pixel.  projective.hpp
// holds the arithmetic; this file holds
//   proj_vertex_key_kernel / proj_vertex_resolve_kernel    a sweep -> its vertex map, nearest range per pixel
//   proj_normal_map_kernel<K>                              normals from the K x K moments about the sensor
//   proj_model_key_kernel / proj_model_resolve_kernel      every live slot's image moved into the newest frame's view
//   proj_accumulate_kernel                                 association at the pixel, rejection, Huber weights, the sums
//                                                          of the normal equations in icp_solve_kernel's row layout
//   proj_map_copy_kernel / proj_map_book_kernel            the handover: the new frame into its slot, poses re-based
// The z-buffers are a 64-bit atomicMin on a key image (projective.hpp: proj_key): the minimum does not depend on the order
// of arrival, so two runs give the same bits.  No other atomic, every loop is bounded, nothing is sized from the data.
#include <math.h>

#include "common.hpp"
#include "icp.hpp"
#include "projective.hpp"

namespace pwclo {

constexpr int PROJ_MAX_SLOTS = 64;          // icp.hip: ICP_MAX_SLOTS
constexpr int PROJ_TILE_W = 32, PROJ_TILE_H = 8;

// points (S, R, C) with C = 3 | 4; lengths (S) or nullptr; keep (S, R) or nullptr -> keys (S, H * W), preset to all ones.
__global__ __launch_bounds__(256) void proj_vertex_key_kernel(ProjImage im, int R, int C, const float *__restrict__ points,
                                                              const int *__restrict__ lengths,
                                                              const int *__restrict__ keep,
                                                              unsigned long long *__restrict__ keys) {
  const int s = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  const int len = lengths != nullptr ? min(max(lengths[s], 0), R) : R;
  if (i >= len) return;
  if (keep != nullptr && keep[(size_t)s * R + i] == 0) return;
  const float *p = points + ((size_t)s * R + i) * C;
  float r;
  int row, col;
  if (!proj_pixel(im, p[0], p[1], p[2], &r, &row, &col)) return;
  atomicMin(keys + (size_t)s * im.H * im.W + (size_t)row * im.W + col, proj_key(r, (unsigned int)i));
}

// keys (S, HW) -> vmap (S, HW, 3), rows (S, HW): the winner's row of points, -1 and the zero vector for an empty pixel.
__global__ __launch_bounds__(256) void proj_vertex_resolve_kernel(int HW, int R, int C, const float *__restrict__ points,
                                                                  const unsigned long long *__restrict__ keys,
                                                                  float *__restrict__ vmap, int *__restrict__ rows) {
  const int s = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  const unsigned long long key = keys[(size_t)s * HW + i];
  float v[3] = {0.0f, 0.0f, 0.0f};
  int row = -1;
  if (key != PROJ_EMPTY_KEY) {
    row = min((int)(key & 0xffffffffull), R - 1);
    const float *p = points + ((size_t)s * R + row) * C;
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
  }
  float *o = vmap + ((size_t)s * HW + i) * 3;
  o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
  rows[(size_t)s * HW + i] = row;
}

// vmap (B, H, W, 3) -> nmap (B, H, W, 3).  One thread per pixel of a PROJ_TILE_H x PROJ_TILE_W tile; the tile and its
// border of K / 2 pixels (zero outside the image) are staged in LDS once, so the image is read about once, not K * K times.
template <int K>
__global__ __launch_bounds__(PROJ_TILE_W *PROJ_TILE_H) void proj_normal_map_kernel(int H, int W,
                                                                                  const float *__restrict__ vmap,
                                                                                  float *__restrict__ nmap) {
  constexpr int HALF = K / 2, LW = PROJ_TILE_W + K - 1, LH = PROJ_TILE_H + K - 1;
  __shared__ float tile[LH][LW][3];
  const int b = blockIdx.z, x0 = blockIdx.x * PROJ_TILE_W, y0 = blockIdx.y * PROJ_TILE_H;
  const float *img = vmap + (size_t)b * H * W * 3;
  for (int e = threadIdx.x; e < LH * LW; e += PROJ_TILE_W * PROJ_TILE_H) {
    const int ly = e / LW, lx = e - ly * LW, y = y0 + ly - HALF, x = x0 + lx - HALF;
    float v[3] = {0.0f, 0.0f, 0.0f};
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const float *p = img + ((size_t)y * W + x) * 3;
      v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
    }
    tile[ly][lx][0] = v[0]; tile[ly][lx][1] = v[1]; tile[ly][lx][2] = v[2];
  }
  __syncthreads();
  const int tx = threadIdx.x % PROJ_TILE_W, ty = threadIdx.x / PROJ_TILE_W, x = x0 + tx, y = y0 + ty;
  if (x >= W || y >= H) return;
  double m[3] = {0.0, 0.0, 0.0}, c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int dy = 0; dy < K; ++dy)
#pragma unroll
    for (int dx = 0; dx < K; ++dx) {
      const double px = tile[ty + dy][tx + dx][0], py = tile[ty + dy][tx + dx][1], pz = tile[ty + dy][tx + dx][2];
      m[0] += px; m[1] += py; m[2] += pz;
      c[0] += px * px; c[1] += px * py; c[2] += px * pz;
      c[3] += py * py; c[4] += py * pz; c[5] += pz * pz;
    }
  float n[3];
  proj_normal(m, c, n);
  const float cx = tile[ty + HALF][tx + HALF][0], cy = tile[ty + HALF][tx + HALF][1], cz = tile[ty + HALF][tx + HALF][2];
  if (cx == 0.0f && cy == 0.0f && cz == 0.0f) {
    n[0] = 0.0f; n[1] = 0.0f; n[2] = 0.0f;
  }
  float *o = nmap + (((size_t)b * H + y) * W + x) * 3;
  o[0] = n[0]; o[1] = n[1]; o[2] = n[2];
}

// The pose that moves slot (s, m)'s points into the newest frame: the rigid inverse of A[s, m] (newest frame -> slot).
__device__ static inline Se3 proj_slot_pose(const double *__restrict__ A, size_t sm) {
  return se3_rigid_inv(se3_load(A + sm * 16));
}

// map_v (S, M, HW, 3), A (S, M, 4, 4), live (S, M) -> keys (S, M, HW), preset to all ones.  A dead slot adds nothing.
__global__ __launch_bounds__(256) void proj_model_key_kernel(ProjImage im, const float *__restrict__ map_v,
                                                             const double *__restrict__ A, const int *__restrict__ live,
                                                             unsigned long long *__restrict__ keys) {
  const int HW = im.H * im.W, sm = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (live[sm] == 0 || i >= HW) return;
  const float *pr = map_v + ((size_t)sm * HW + i) * 3;
  const float p[3] = {pr[0], pr[1], pr[2]};
  if (p[0] == 0.0f && p[1] == 0.0f && p[2] == 0.0f) return;
  double o[3];
  se3_apply(proj_slot_pose(A, (size_t)sm), p, o);
  float r;
  int row, col;
  if (!proj_pixel(im, (float)o[0], (float)o[1], (float)o[2], &r, &row, &col)) return;
  atomicMin(keys + (size_t)sm * HW + (size_t)row * im.W + col, proj_key(r, (unsigned int)i));
}

// keys -> model_v, model_n (S, M, HW, 3) and src (S, M, HW): the slot's pixel that won (-1: empty; a dead slot is empty).
__global__ __launch_bounds__(256) void proj_model_resolve_kernel(int HW, const float *__restrict__ map_v,
                                                                 const float *__restrict__ map_n,
                                                                 const double *__restrict__ A, const int *__restrict__ live,
                                                                 const unsigned long long *__restrict__ keys,
                                                                 float *__restrict__ model_v, float *__restrict__ model_n,
                                                                 int *__restrict__ src) {
  const int sm = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  float v[3] = {0.0f, 0.0f, 0.0f}, n[3] = {0.0f, 0.0f, 0.0f};
  int from = -1;
  const unsigned long long key = live[sm] != 0 ? keys[(size_t)sm * HW + i] : PROJ_EMPTY_KEY;
  if (key != PROJ_EMPTY_KEY) {
    from = min((int)(key & 0xffffffffull), HW - 1);
    const float *pr = map_v + ((size_t)sm * HW + from) * 3, *nr = map_n + ((size_t)sm * HW + from) * 3;
    const float p[3] = {pr[0], pr[1], pr[2]};
    const double nd[3] = {nr[0], nr[1], nr[2]};
    const Se3 inv = proj_slot_pose(A, (size_t)sm);
    double o[3], on[3];
    se3_apply(inv, p, o);
    se3_rotate(inv, nd, on);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      v[a] = (float)o[a];
      n[a] = (float)on[a];
    }
  }
  float *vo = model_v + ((size_t)sm * HW + i) * 3, *no = model_n + ((size_t)sm * HW + i) * 3;
  vo[0] = v[0]; vo[1] = v[1]; vo[2] = v[2];
  no[0] = n[0]; no[1] = n[1]; no[2] = n[2];
  src[(size_t)sm * HW + i] = from;
}

// vmap (S, HW, 3): the new frame's own vertex map, one thread per pixel; model_v / model_n (S, M, HW, 3); T (S, 4, 4)
// -> partial (S, gridDim.x, ICP_ROW), and for tests slot / pixel (S, HW) or nullptr.
__global__ __launch_bounds__(ICP_ACC_THREADS) void proj_accumulate_kernel(
    ProjImage im, int M, const float *__restrict__ vmap, const float *__restrict__ model_v,
    const float *__restrict__ model_n, const double *__restrict__ T, double sigma, float max_dist,
    double *__restrict__ partial, int *__restrict__ slot_out, int *__restrict__ pixel_out) {
  const int HW = im.H * im.W, s = blockIdx.y, i = blockIdx.x * ICP_ACC_THREADS + threadIdx.x;
  double acc[ICP_TERMS];
#pragma unroll
  for (int e = 0; e < ICP_TERMS; ++e) acc[e] = 0.0;
  if (i < HW) {
    int best = -1, pixel = -1;
    const float *pr = vmap + ((size_t)s * HW + i) * 3;
    const float p[3] = {pr[0], pr[1], pr[2]};
    if (p[0] != 0.0f || p[1] != 0.0f || p[2] != 0.0f) {
      const Se3 t = se3_load(T + (size_t)s * 16);
      double o[3];
      se3_apply(t, p, o);
      const float q[3] = {(float)o[0], (float)o[1], (float)o[2]};
      float r;
      int row, col;
      if (proj_pixel(im, q[0], q[1], q[2], &r, &row, &col)) {
        pixel = row * im.W + col;
        float bd = 0.0f, y[3] = {0.0f, 0.0f, 0.0f};
        for (int m = 0; m < M; ++m) {
          const float *yr = model_v + (((size_t)s * M + m) * HW + pixel) * 3;
          const float c[3] = {yr[0], yr[1], yr[2]};
          if (c[0] == 0.0f && c[1] == 0.0f && c[2] == 0.0f) continue;
          const float dx = q[0] - c[0], dy = q[1] - c[1], dz = q[2] - c[2];
          const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
          if (best < 0 || d < bd) {                         // strict: on a tie the lower slot stays
            best = m;
            bd = d;
            y[0] = c[0]; y[1] = c[1]; y[2] = c[2];
          }
        }
        if (best >= 0 && !(bd <= max_dist)) best = -1;      // NaN fails
        if (best >= 0) {
          const float *nr = model_n + (((size_t)s * M + best) * HW + pixel) * 3;
          const float nn[3] = {nr[0], nr[1], nr[2]};
          if (nn[0] != 0.0f || nn[1] != 0.0f || nn[2] != 0.0f) {
            const double eye[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};   // the model is in the previous frame
            icp_add_pair(p, q, y, nn, t, eye, sigma, acc);
          } else {
            best = -1;
          }
        }
      }
    }
    if (slot_out != nullptr) slot_out[(size_t)s * HW + i] = best;
    if (pixel_out != nullptr) pixel_out[(size_t)s * HW + i] = pixel;
  }
  icp_reduce_store_row(acc, partial, s);
}

// The new frame's images (S, HW3) into slot cursor[s] of map_v / map_n (S, M, HW3).  Reads the cursor, never writes it.
__global__ __launch_bounds__(256) void proj_map_copy_kernel(int M, int HW3, const float *__restrict__ vmap,
                                                            const float *__restrict__ nmap, float *__restrict__ map_v,
                                                            float *__restrict__ map_n, const int *__restrict__ cursor) {
  const int s = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j >= HW3) return;
  const int slot = min(max(cursor[s], 0), M - 1);
  const size_t dst = ((size_t)s * M + slot) * HW3 + j, from = (size_t)s * HW3 + j;
  map_v[dst] = vmap[from];
  map_n[dst] = nmap[from];
}

// icp_map_push_kernel's bookkeeping without the search structures and without Rm (icp.hpp: icp_slot_after_push), then the
// cursor moves on.  One workgroup per stream, one thread per slot.
__global__ __launch_bounds__(PROJ_MAX_SLOTS) void proj_map_book_kernel(int M, const double *__restrict__ T,
                                                                       double *__restrict__ A, int *__restrict__ live,
                                                                       int *__restrict__ cursor) {
  const int s = blockIdx.x, m = threadIdx.x;
  const int slot = min(max(cursor[s], 0), M - 1);
  if (m < M) icp_slot_after_push(m == slot, live + s * M + m, A + ((size_t)s * M + m) * 16, T + (size_t)s * 16, nullptr);
  __syncthreads();                                         // everyone has read the cursor
  if (threadIdx.x == 0) cursor[s] = slot + 1 == M ? 0 : slot + 1;
}

}  // namespace pwclo

using namespace pwclo;

static bool proj_image_ok(int H, int W, double up_fov, double down_fov) {
  return H >= 1 && W >= 1 && (long long)H * W * 3 < (1ll << 31) && isfinite(up_fov) && isfinite(down_fov) &&
         fabs(up_fov) + fabs(down_fov) > 0.0;
}

// Presets a key image to all ones on the launch stream; false (and a sticky error) if the runtime refuses.
static bool proj_preset_keys(const char *what, void *keys, long long count) {
  const hipError_t e = hipMemsetAsync(keys, 0xff, (size_t)count * 8, current_stream());
  if (e != hipSuccess) {
    set_error(PWCLO_EINVAL, "%s: presetting the key image failed: %s", what, hipGetErrorString(e));
    return false;
  }
  return true;
}

extern "C" long long proj_vertex_map_workspace_bytes(int S, int H, int W) {
  return S >= 1 && H >= 1 && W >= 1 ? (long long)S * H * W * 8 : 0;
}

extern "C" void proj_vertex_map_kernel_wrapper(int S, int R, int C, int H, int W, double up_fov, double down_fov,
                                               const float *points, const int *lengths, const int *keep, void *workspace,
                                               float *vmap, int *rows) {
  if (S <= 0) return;
  PWCLO_REQUIRE(proj_image_ok(H, W, up_fov, down_fov), "proj_vertex_map: H=%d W=%d up_fov=%g down_fov=%g out of range", H,
                W, up_fov, down_fov);
  PWCLO_REQUIRE(R >= 1 && (C == 3 || C == 4) && (long long)R * C < (1ll << 31) && S <= 65535,
                "proj_vertex_map: S=%d R=%d C=%d out of range (C = 3 or 4)", S, R, C);
  PWCLO_REQUIRE(points != nullptr && workspace != nullptr && vmap != nullptr && rows != nullptr &&
                aligned(workspace, 8), "proj_vertex_map: points, workspace (8-byte aligned), vmap and rows are required%s",
                "");
  const ProjImage im = proj_image(H, W, up_fov, down_fov);
  unsigned long long *keys = static_cast<unsigned long long *>(workspace);
  if (!proj_preset_keys("proj_vertex_map", keys, (long long)S * H * W)) return;
  hipLaunchKernelGGL(proj_vertex_key_kernel, dim3(ceil_div(R, 256), S), dim3(256), 0, current_stream(), im, R, C, points,
                     lengths, keep, keys);
  if (!check_launch("proj_vertex_map (keys)")) return;
  hipLaunchKernelGGL(proj_vertex_resolve_kernel, dim3(ceil_div(H * W, 256), S), dim3(256), 0, current_stream(), H * W, R, C,
                     points, keys, vmap, rows);
  check_launch("proj_vertex_map");
}

extern "C" void proj_normal_map_kernel_wrapper(int B, int H, int W, int kernel_size, const float *vmap, float *nmap) {
  if (B <= 0) return;
  PWCLO_REQUIRE(H >= 1 && W >= 1 && (long long)H * W * 3 < (1ll << 31) && B <= 65535 && ceil_div(H, PROJ_TILE_H) <= 65535,
                "proj_normal_map: B=%d H=%d W=%d out of range", B, H, W);
  PWCLO_REQUIRE(kernel_size == 3 || kernel_size == 5, "proj_normal_map: kernel_size=%d is not instantiated (3 or 5)",
                kernel_size);
  PWCLO_REQUIRE(vmap != nullptr && nmap != nullptr && vmap != nmap, "proj_normal_map: vmap and nmap (distinct) are required%s",
                "");
  const dim3 grid(ceil_div(W, PROJ_TILE_W), ceil_div(H, PROJ_TILE_H), B), block(PROJ_TILE_W * PROJ_TILE_H);
  if (kernel_size == 3)
    hipLaunchKernelGGL(proj_normal_map_kernel<3>, grid, block, 0, current_stream(), H, W, vmap, nmap);
  else
    hipLaunchKernelGGL(proj_normal_map_kernel<5>, grid, block, 0, current_stream(), H, W, vmap, nmap);
  check_launch("proj_normal_map");
}

extern "C" long long proj_model_build_workspace_bytes(int S, int M, int H, int W) {
  return S >= 1 && M >= 1 && H >= 1 && W >= 1 ? (long long)S * M * H * W * 8 : 0;
}

extern "C" void proj_model_build_kernel_wrapper(int S, int M, int H, int W, double up_fov, double down_fov,
                                                const float *map_v, const float *map_n, const double *A, const int *live,
                                                void *workspace, float *model_v, float *model_n, int *src) {
  if (S <= 0) return;
  PWCLO_REQUIRE(proj_image_ok(H, W, up_fov, down_fov), "proj_model_build: H=%d W=%d up_fov=%g down_fov=%g out of range", H,
                W, up_fov, down_fov);
  PWCLO_REQUIRE(M >= 1 && M <= PROJ_MAX_SLOTS && (long long)S * M <= 65535 &&
                (long long)S * M * H * W * 3 < (1ll << 40), "proj_model_build: S=%d M=%d out of range (M <= %d, S * M <= 65535)",
                S, M, PROJ_MAX_SLOTS);
  PWCLO_REQUIRE(map_v != nullptr && map_n != nullptr && A != nullptr && live != nullptr && workspace != nullptr &&
                model_v != nullptr && model_n != nullptr && src != nullptr, "proj_model_build: every pointer is required%s",
                "");
  PWCLO_REQUIRE(aligned(A, 8) && aligned(workspace, 8), "proj_model_build: A and workspace must be 8-byte aligned%s",
                "");
  const ProjImage im = proj_image(H, W, up_fov, down_fov);
  unsigned long long *keys = static_cast<unsigned long long *>(workspace);
  if (!proj_preset_keys("proj_model_build", keys, (long long)S * M * H * W)) return;
  const dim3 grid(ceil_div(H * W, 256), S * M);
  hipLaunchKernelGGL(proj_model_key_kernel, grid, dim3(256), 0, current_stream(), im, map_v, A, live, keys);
  if (!check_launch("proj_model_build (keys)")) return;
  hipLaunchKernelGGL(proj_model_resolve_kernel, grid, dim3(256), 0, current_stream(), H * W, map_v, map_n, A, live, keys,
                     model_v, model_n, src);
  check_launch("proj_model_build");
}

extern "C" void proj_accumulate_kernel_wrapper(int S, int M, int H, int W, double up_fov, double down_fov, const float *vmap,
                                               const float *model_v, const float *model_n, const double *T, double sigma,
                                               float max_dist, double *partial, int *slot, int *pixel) {
  if (S <= 0) return;
  PWCLO_REQUIRE(proj_image_ok(H, W, up_fov, down_fov), "proj_accumulate: H=%d W=%d up_fov=%g down_fov=%g out of range", H, W,
                up_fov, down_fov);
  PWCLO_REQUIRE(M >= 1 && M <= PROJ_MAX_SLOTS && S <= 65535, "proj_accumulate: S=%d M=%d out of range (M <= %d)", S, M,
                PROJ_MAX_SLOTS);
  PWCLO_REQUIRE(sigma > 0.0 && isfinite(sigma) && max_dist >= 0.0f, "proj_accumulate: sigma=%g must be > 0, max_dist=%g >= 0",
                sigma, (double)max_dist);
  PWCLO_REQUIRE(vmap != nullptr && model_v != nullptr && model_n != nullptr && T != nullptr && partial != nullptr,
                "proj_accumulate: every pointer but slot and pixel is required%s", "");
  PWCLO_REQUIRE(aligned(T, 8) && aligned(partial, 8), "proj_accumulate: T and partial must be 8-byte aligned%s", "");
  const ProjImage im = proj_image(H, W, up_fov, down_fov);
  hipLaunchKernelGGL(proj_accumulate_kernel, dim3(icp_accumulate_groups(H * W), S), dim3(ICP_ACC_THREADS), 0,
                     current_stream(), im, M, vmap, model_v, model_n, T, sigma, max_dist, partial, slot, pixel);
  check_launch("proj_accumulate");
}

extern "C" void proj_map_push_kernel_wrapper(int S, int M, int H, int W, const double *T, const float *vmap,
                                             const float *nmap, float *map_v, float *map_n, double *A, int *live,
                                             int *cursor) {
  if (S <= 0) return;
  PWCLO_REQUIRE(H >= 1 && W >= 1 && (long long)H * W * 3 < (1ll << 31) && M >= 1 && M <= PROJ_MAX_SLOTS && S <= 65535,
                "proj_map_push: S=%d M=%d H=%d W=%d out of range (M <= %d)", S, M, H, W, PROJ_MAX_SLOTS);
  PWCLO_REQUIRE(T != nullptr && vmap != nullptr && nmap != nullptr && map_v != nullptr && map_n != nullptr && A != nullptr &&
                live != nullptr && cursor != nullptr, "proj_map_push: every pointer is required%s", "");
  PWCLO_REQUIRE(aligned(T, 8) && aligned(A, 8), "proj_map_push: T and A must be 8-byte aligned%s", "");
  const int HW3 = H * W * 3;
  hipLaunchKernelGGL(proj_map_copy_kernel, dim3(ceil_div(HW3, 256), S), dim3(256), 0, current_stream(), M, HW3, vmap, nmap,
                     map_v, map_n, cursor);
  if (!check_launch("proj_map_push (copy)")) return;
  hipLaunchKernelGGL(proj_map_book_kernel, dim3(S), dim3(PROJ_MAX_SLOTS), 0, current_stream(), M, T, A, live, cursor);
  check_launch("proj_map_push");
}
