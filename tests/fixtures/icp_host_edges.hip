// Prints, as hex bit patterns, what the host+device arithmetic of csrc/icp.hpp computes on the edge inputs of
// tests/icp_cases.py: icp_eig3 and icp_normal, icp_huber_w2 and icp_add_pair, icp_solve6 and icp_update_pose.  A stand-alone
// host program (never loaded into Python), built with the sanitizers on the host side only:
//
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -ffp-contract=off -fno-fast-math -Xarch_host -fsanitize=address,undefined \
//         -I pwclonet_pylidarslam_amd/csrc tests/fixtures/icp_host_edges.hip -o icp_host_edges && ./icp_host_edges
//
// tests/test_icp_host_edges_cpu.py builds it, runs it once and compares every line with tests/icp_model.py.  One line per
// result: a label, an index, then the words.  The inputs are printed too ("in_..." lines), and the test requires them to be
// its own tables bit for bit, so the two files cannot drift apart unseen.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "se3.hpp"
#include "icp.hpp"

using namespace pwclo;

static void put(const char *label, int i, const double *v, int n) {
  printf("%s %d", label, i);
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

int main() {
  const double nan = NAN;
  // ---- icp_eig3: [xx xy xz yy yz zz] ---------------------------------------------------------------------------------------------
  const double mats[][6] = {
      {3.0, 0.0, 0.0, 1.0, 0.0, 2.0},                       // 0 diagonal
      {0.0, 0.0, 0.0, 0.0, 0.0, 0.0},                       // 1 zero
      {2.0, 0.0, 0.0, 2.0, 0.0, 5.0},                       // 2 two equal eigenvalues, diagonal
      {3.0, 1.0, 1.0, 3.0, 1.0, 3.0},                       // 3 two equal eigenvalues (2, 2, 5), not diagonal
      {1.0, nan, 0.0, 2.0, 0.0, 3.0},                       // 4 a NaN entry off the diagonal
      {nan, 0.5, 0.0, 2.0, 0.0, 3.0},                       // 5 a NaN entry on the diagonal
      {1e30, 2e29, -3e29, 4e30, 5e29, 9e30},                // 6 entries of 1e30
      {84.0, -42.0, 0.0, 84.0, 0.0, 0.0},                   // 7 an exactly planar neighbourhood in z = 0
      {4.0, 1.0, -2.0, 3.0, 0.5, 6.0},                      // 8 general
      {1.0, 1e-9, 0.0, 1e-18, 0.0, 0.0},                    // 9 rank one up to rounding
  };
  const int NM = (int)(sizeof(mats) / sizeof(mats[0]));
  const float ys[][3] = {{1.0f, 2.0f, 8.0f}, {0.0f, 0.0f, 0.0f}, {-1.0f, -2.0f, -8.0f}};
  for (int k = 0; k < 3; ++k) putf("in_y", k, ys[k], 3);
  for (int i = 0; i < NM; ++i) {
    double val[3], vec[3];
    put("in_mat", i, mats[i], 6);
    icp_eig3(mats[i], val, vec);
    put("eig_val", i, val, 3);
    put("eig_vec", i, vec, 3);
    for (int k = 0; k < 3; ++k) {
      float out[3];
      double eig[3];
      icp_normal(mats[i], ys[k], out, eig);
      putf("normal", 3 * i + k, out, 3);
    }
  }
  // ---- icp_huber_w2 -----------------------------------------------------------------------------------------------------------------
  const float s3 = 0.3f;
  const double hub[][2] = {                                 // (r, sigma)
      {(double)s3, (double)s3}, {-(double)s3, (double)s3}, {0.0, 0.5}, {-0.0, 0.5}, {0.25, 0.5}, {0.75, 0.5},
      {(double)6e-5f, 5e-5}, {(double)1e-4f, 5e-5}, {(double)2e-4f, 5e-5}, {-(double)6e-5f, 5e-5}, {(double)4e-5f, 5e-5},
      {1e-4, 5e-5}, {nan, 0.5}, {INFINITY, 0.5}, {5e-5, 5e-5},
  };
  const int NH = (int)(sizeof(hub) / sizeof(hub[0]));
  for (int i = 0; i < NH; ++i) {
    put("in_huber", i, hub[i], 2);
    const double w = icp_huber_w2(hub[i][0], hub[i][1]);
    put("huber", i, &w, 1);
  }
  // ---- icp_add_pair: the planted residuals of the accumulate cases (map point (1, 2, 0), normal (0, 0, 1)) ------------------------
  const Se3 T = {{0.9987502603949663, -0.04997916927067833, 0.0, 0.1, 0.04997916927067833, 0.9987502603949663, 0.0, -0.2, 0.0,
                  0.0, 1.0, 0.05}};
  const double Rm[9] = {0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0};
  const float p[3] = {1.5f, -2.25f, 0.75f}, y[3] = {1.0f, 2.0f, 0.0f}, n[3] = {0.0f, 0.0f, 1.0f};
  const float n2[3] = {0.36f, -0.48f, 0.8f};
  const double pairs[][2] = {{(double)s3, (double)s3}, {-(double)s3, (double)s3}, {0.0, 0.5}, {(double)6e-5f, 5e-5},
                             {(double)1e-4f, 5e-5}, {(double)2e-4f, 5e-5}, {0.25, 0.5}, {3.0, 0.5}};
  const int NP = (int)(sizeof(pairs) / sizeof(pairs[0]));
  put("in_T", 0, T.m, 12);
  put("in_Rm", 0, Rm, 9);
  putf("in_p", 0, p, 3);
  putf("in_map", 0, y, 3);
  putf("in_n", 0, n, 3);
  putf("in_n", 1, n2, 3);
  double acc[ICP_TERMS], all[ICP_TERMS];
  for (int e = 0; e < ICP_TERMS; ++e) all[e] = 0.0;
  for (int i = 0; i < NP; ++i) {
    const float q[3] = {1.0f, 2.0f, (float)pairs[i][0]};
    for (int e = 0; e < ICP_TERMS; ++e) acc[e] = 0.0;
    put("in_pair", i, pairs[i], 2);
    putf("in_q", i, q, 3);
    icp_add_pair(p, q, y, n, T, Rm, pairs[i][1], acc);
    put("pair", i, acc, ICP_TERMS);
    const float q2[3] = {1.25f, 1.5f, (float)pairs[i][0]};
    putf("in_q2", i, q2, 3);
    icp_add_pair(p, q2, y, n2, T, Rm, 0.5, all);
  }
  put("pair_sum", 0, all, ICP_TERMS);
  // ---- icp_solve6 and icp_update_pose -------------------------------------------------------------------------------------------------
  double rows[8][ICP_ROW];
  for (int i = 0; i < 8; ++i)
    for (int e = 0; e < ICP_ROW; ++e) rows[i][e] = 0.0;
  const double step345[6] = {0.0, 0.0, 0.0, 3.0 / 1024, 4.0 / 1024, 0.0};
  const double th = 3.141592653589793 - 5e-7;
  const double nearpi[6] = {th / 3.0, 2.0 * th / 3.0, 2.0 * th / 3.0, 0.1, -0.2, 0.3};
  for (int i = 0; i < 8; ++i) {                            // 0..5: sw = 1, H = 4 I: pivots of 2, an exact solve
    int e = 0;
    for (int a = 0; a < 6; ++a)
      for (int b = a; b < 6; ++b) rows[i][ICP_H + e++] = a == b ? 4.0 : 0.0;
    rows[i][ICP_SW] = 1.0;
    rows[i][ICP_PAIRS] = 400.0;
  }
  for (int a = 0; a < 6; ++a) {
    rows[0][ICP_G + a] = -4.0 * step345[a];
    rows[1][ICP_G + a] = -4.0 * nearpi[a];
    rows[3][ICP_G + a] = 0.5 * (a + 1);
    rows[4][ICP_G + a] = 0.5 * (a + 1);
    rows[5][ICP_G + a] = 0.5 * (a + 1);
    rows[7][ICP_G + a] = 0.25 * (a - 2);
  }
  rows[3][ICP_H + 7] = nan;                                 // 2: g = 0;  3, 4, 5: a NaN in H, in g, in sw
  rows[4][ICP_G + 2] = nan;
  rows[5][ICP_SW] = nan;
  for (int e = 0; e < ICP_TERMS; ++e) rows[6][e] = 0.0;    // 6: the one pair with J = (0, 0, 0, 0, 0, 1), r = 0.25
  rows[6][ICP_H + 20] = 1.0;
  rows[6][ICP_G + 5] = 0.25;
  rows[6][ICP_SW] = 1.0;
  rows[6][ICP_COST] = 0.0625;
  rows[6][ICP_PAIRS] = 1.0;
  rows[7][ICP_H + 1] = 1.0;                                 // 7: general, coupled
  rows[7][ICP_H + 9] = -0.5;
  const double dampings[2] = {0.0, 1e-6};
  put("in_damping", 0, dampings, 2);
  for (int i = 0; i < 8; ++i) put("in_row", i, rows[i], ICP_ROW);
  for (int i = 0; i < 8; ++i)
    for (int d = 0; d < 2; ++d) {
      double delta[6] = {7.0, 7.0, 7.0, 7.0, 7.0, 7.0};    // untouched when the solve is refused
      const double ok = icp_solve6(rows[i], dampings[d], delta) ? 1.0 : 0.0;
      put("solve_ok", 2 * i + d, &ok, 1);
      put("solve", 2 * i + d, delta, 6);
      if (ok != 0.0) {
        Se3 t = T;
        icp_update_pose(delta, t);
        put("update", 2 * i + d, t.m, 12);
      }
    }
  const double zero[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  Se3 t = T;
  icp_update_pose(zero, t);                                 // th == 0: the re-orthonormalisation alone
  put("update_zero", 0, t.m, 12);
  return 0;
}
