// Prints, as hex bit patterns, what the host+device arithmetic of csrc/se3.hpp and csrc/icp.hpp computes on a fixed table
// of poses, points and twists.  A stand-alone host program (never loaded into Python): two trees whose outputs are
// byte-identical compute the same bits in se3_mul, se3_rigid_inv, se3_apply, se3_rotate, se3_quat, se3_to_pose_row,
// icp_add_pair, icp_solve6 and icp_update_pose.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -Xarch_host -fsanitize=address,undefined \
//         -I pwclonet_pylidarslam_amd/csrc tests/fixtures/se3_bits.hip -o se3_bits && ./se3_bits | sha256sum
//
// -DSE3_BITS_OLD_NAMES builds the same program against a tree from before se3.hpp became the only home of this arithmetic
// (icp_pose_mul / icp_pose_apply on double[12], proj_pose_inverse, pg_rigid_inv, pg_quat); there the functions that
// existed twice are also required to agree with each other.  Those trees qualify se3.hpp and pose_graph.hpp __device__
// only: give the compiler copies of the two headers with __host__ added (profiles/se3_unify/README.md has the commands).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "se3.hpp"
#include "icp.hpp"
#ifdef SE3_BITS_OLD_NAMES
#include "projective.hpp"
#include "pose_graph.hpp"
#endif

using namespace pwclo;

static void same(const double *a, const double *b, int n, const char *what) {
  if (memcmp(a, b, sizeof(double) * n) != 0) {
    fprintf(stderr, "the two old definitions of %s disagree\n", what);
    exit(2);
  }
}

#ifdef SE3_BITS_OLD_NAMES
struct Quat { double w, x, y, z; };
static Se3 v_mul(const Se3 &a, const Se3 &b) {
  Se3 c;
  icp_pose_mul(a.m, b.m, c.m);
  const Se3 d = se3_mul(a, b);
  same(c.m, d.m, 12, "the product");
  return c;
}
static Se3 v_rigid_inv(const Se3 &a) {
  Se3 r;
  proj_pose_inverse(a.m, r.m);
  const Se3 d = pg_rigid_inv(a);
  same(r.m, d.m, 12, "the rigid inverse");
  return r;
}
static void v_apply(const Se3 &a, const float p[3], double o[3]) { icp_pose_apply(a.m, p, o); }
static void v_rotate(const Se3 &a, const double v[3], double o[3]) {      // the two resolve kernels' expression
  for (int i = 0; i < 3; ++i) o[i] = (a.m[4 * i] * v[0] + a.m[4 * i + 1] * v[1]) + a.m[4 * i + 2] * v[2];
}
static Quat v_quat(const Se3 &a) {
  const PgQuat q = pg_quat(a);
  return Quat{q.w, q.x, q.y, q.z};
}
static void v_add_pair(const float p[3], const float q[3], const float y[3], const float n[3], const Se3 &T,
                       const double Rm[9], double sigma, double acc[ICP_TERMS]) {
  icp_add_pair(p, q, y, n, T.m, Rm, sigma, acc);
}
static void v_update(const double delta[6], Se3 &T) { icp_update_pose(delta, T.m); }
#else
static Se3 v_mul(const Se3 &a, const Se3 &b) { return se3_mul(a, b); }
static Se3 v_rigid_inv(const Se3 &a) { return se3_rigid_inv(a); }
static void v_apply(const Se3 &a, const float p[3], double o[3]) { se3_apply(a, p, o); }
static void v_rotate(const Se3 &a, const double v[3], double o[3]) { se3_rotate(a, v, o); }
static Quat v_quat(const Se3 &a) { return se3_quat(a); }
static void v_add_pair(const float p[3], const float q[3], const float y[3], const float n[3], const Se3 &T,
                       const double Rm[9], double sigma, double acc[ICP_TERMS]) {
  icp_add_pair(p, q, y, n, T, Rm, sigma, acc);
}
static void v_update(const double delta[6], Se3 &T) { icp_update_pose(delta, T); }
#endif

static void put(const char *label, int i, int j, const double *v, int n) {
  printf("%s %d %d", label, i, j);
  for (int e = 0; e < n; ++e) {
    unsigned long long b;
    memcpy(&b, &v[e], 8);
    printf(" %016llx", b);
  }
  printf("\n");
}
static void putf(const char *label, int i, const float *v, int n) {
  printf("%s %d", label, i);
  for (int e = 0; e < n; ++e) {
    unsigned int b;
    memcpy(&b, &v[e], 4);
    printf(" %08x", b);
  }
  printf("\n");
}

static unsigned int lcg_state = 12345u;
static float lcg(float lo, float hi) {                                     // a fixed stream of fp32 values in [lo, hi)
  lcg_state = lcg_state * 1664525u + 1013904223u;
  return lo + (hi - lo) * (float)(lcg_state >> 8) * (1.0f / 16777216.0f);
}

int main() {
  const double c3 = -0.9899924966004454, s3 = 0.1411200080598672;          // cos, sin of 3 rad: close to pi, both signs of w
  const float row[7] = {0.3f, -1.2f, 2.5f, 0.8f, 0.1f, -0.5f, 0.3f};       // a general pose from a non-unit quaternion
  const Se3 table[] = {
      se3_identity(),
      {{1, 0, 0, 0.5, 0, -1, 0, -2.0, 0, 0, -1, 0.25}},                    // exactly pi about x, y, z: the three diagonal
      {{-1, 0, 0, 1.5, 0, 1, 0, 0.125, 0, 0, -1, -3.0}},                   // branches of Shepperd's selection
      {{-1, 0, 0, -0.75, 0, -1, 0, 4.0, 0, 0, 1, 0.0}},
      {{1, 0, 0, 0.1, 0, c3, -s3, 0.2, 0, s3, c3, 0.3}},                   // 3 rad and -3 rad about each axis
      {{1, 0, 0, 0.1, 0, c3, s3, 0.2, 0, -s3, c3, 0.3}},
      {{c3, 0, s3, -1.0, 0, 1, 0, 2.0, -s3, 0, c3, -3.0}},
      {{c3, 0, -s3, -1.0, 0, 1, 0, 2.0, s3, 0, c3, -3.0}},
      {{c3, -s3, 0, 7.0, s3, c3, 0, -8.0, 0, 0, 1, 9.0}},
      {{c3, s3, 0, 7.0, -s3, c3, 0, -8.0, 0, 0, 1, 9.0}},
      {{0, -1, 0, 10.0, 1, 0, 0, -20.0, 0, 0, 1, 30.0}},                   // a quarter turn about z
      pose_row_to_se3(row),
      {{0.9, 0.2, -0.1, 1.0, -0.3, 1.1, 0.4, -2.0, 0.05, -0.6, 0.7, 3.0}},  // not orthonormal
      {{2.0, 0, 0, 0, 0, -3.0, 0, 0, 0, 0, 0.5, 0}},                        // a scaling with a reflection
  };
  const int NT = (int)(sizeof(table) / sizeof(table[0]));
  const double twists[][6] = {
      {0, 0, 0, 0, 0, 0},
      {1e-12, 0, 0, 0, 0, 0},
      {0, -1e-12, 1e-12, 1e-12, 0, -1e-12},
      {0.01, -0.02, 0.03, 0.1, -0.2, 0.3},
      {1.5, -2.0, 0.7, -4.0, 5.0, 6.0},
      {0, 0, 3.141592653589793, 0, 0, 0},
  };
  const int NW = (int)(sizeof(twists) / sizeof(twists[0]));
  const float pts[][3] = {{0.0f, 0.0f, 0.0f}, {1.0f, -2.0f, 3.0f}, {-17.25f, 0.001f, 42.5f}, {1e-20f, -1e20f, 3.3f}};
  const int NP = (int)(sizeof(pts) / sizeof(pts[0]));

  for (int i = 0; i < NT; ++i)
    for (int j = 0; j < NT; ++j) put("mul", i, j, v_mul(table[i], table[j]).m, 12);
  for (int i = 0; i < NT; ++i) {
    const Se3 &a = table[i];
    put("rigid_inv", i, 0, v_rigid_inv(a).m, 12);
    for (int k = 0; k < NP; ++k) {
      double o[3], on[3];
      const double d[3] = {pts[k][0], pts[k][1], pts[k][2]};
      v_apply(a, pts[k], o);
      v_rotate(a, d, on);
      put("apply", i, k, o, 3);
      put("rotate", i, k, on, 3);
    }
    const Quat q = v_quat(a);
    const double qd[4] = {q.w, q.x, q.y, q.z};
    put("quat", i, 0, qd, 4);
    float r[7];
    se3_to_pose_row(a, r);
    putf("pose_row", i, r, 7);
  }
  // rows of the normal equations: per pose, 24 pairs from the fixed stream, below and above the Huber threshold
  for (int i = 0; i < NT; ++i) {
    double acc[ICP_TERMS], sum[ICP_ROW], delta[6] = {0, 0, 0, 0, 0, 0};
    for (int e = 0; e < ICP_TERMS; ++e) acc[e] = 0.0;
    const Se3 R = v_rigid_inv(table[(i + 4) % NT]);
    const double Rm[9] = {R.m[0], R.m[1], R.m[2], R.m[4], R.m[5], R.m[6], R.m[8], R.m[9], R.m[10]};
    for (int k = 0; k < 24; ++k) {
      const float p[3] = {lcg(-10, 10), lcg(-10, 10), lcg(-2, 2)}, y[3] = {lcg(-10, 10), lcg(-10, 10), lcg(-2, 2)};
      const float off = k % 3 == 0 ? 2.0f : 0.05f;
      const float q[3] = {y[0] + lcg(-off, off), y[1] + lcg(-off, off), y[2] + lcg(-off, off)};
      const float n[3] = {lcg(-1, 1), lcg(-1, 1), lcg(-1, 1)};
      v_add_pair(p, q, y, n, table[i], Rm, 0.5, acc);
      if (k == 0) put("pair", i, k, acc, ICP_TERMS);
    }
    put("row", i, 0, acc, ICP_TERMS);
    for (int e = 0; e < ICP_ROW; ++e) sum[e] = e < ICP_TERMS ? acc[e] : 0.0;
    const double ok = icp_solve6(sum, 1e-6, delta) ? 1.0 : 0.0;
    put("solve_ok", i, 0, &ok, 1);
    put("solve", i, 0, delta, 6);
    Se3 t = table[i];
    v_update(delta, t);
    put("solve_update", i, 0, t.m, 12);
    sum[ICP_H] = -1.0;                                                      // a pivot that is not positive
    const double bad = icp_solve6(sum, 0.0, delta) ? 1.0 : 0.0;
    put("solve_bad", i, 0, &bad, 1);
  }
  for (int w = 0; w < NW; ++w)
    for (int i = 0; i < NT; ++i) {
      Se3 t = table[i];
      v_update(twists[w], t);
      put("update", w, i, t.m, 12);
    }
  return 0;
}
