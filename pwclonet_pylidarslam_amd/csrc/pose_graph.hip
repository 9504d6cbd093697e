// Pose-graph backend: SE(3) graph optimisation per stream by Levenberg-Marquardt (gfx950, fp64).
//
// A stream's graph: vertices X (N, S, 4, 4) (count[s] of them in use, vertex 0 the identity), the chain edge k - 1 -> k with
// the measurement Zc[k] for every vertex k >= 1, nloops[s] loop edges (i, j, Z, Omega) and nabs[s] absolute edges (i, G,
// Omega).  Edge ids of a stream: chain edge k at k (id 0 is never an edge), loop l at N + l, absolute edge a at N + ML + a.
// One LM iteration is four launches:
//   linearise  one thread per edge: error, Jacobians and the edge's blocks into its slot (pose_graph.hpp)
//   solve      one workgroup per stream: chi2, the gradient and the block diagonal gathered per vertex, lambda_0 in
//              iteration 0, block-Jacobi preconditioned conjugate gradients on (H + lambda I) delta = -b with every vector
//              in global memory (6 N doubles do not fit LDS at N in the thousands; L2 holds them), delta and the trial poses
//   linearise  again, at the trial poses, chi2 terms only
//   judge      one workgroup per stream: chi2_new, the gain ratio, accept / reject, lambda, the status word; an accepted
//              step copies the trial poses over the vertices
// Every sum is taken in a fixed order (block_sum below), there is no atomic, and no workgroup waits on another.  A stream
// with active[s] == 0, or whose status word is set, is skipped by every kernel but the read-out of the edge weights.  With a
// robust kernel (section 25.1) linearise writes rho(c) as an edge's chi2 term and its blocks and gradients times the weight w.
#include "pose_graph.hpp"

namespace pwclo {

struct PgGraph {
  int S, N, ML, MA, fix_first;
  const int *active, *status, *count, *nloops, *nabs;
  const double *Zc;
  const int *loop_ij;
  const double *loop_Z, *loop_Om;
  const int *abs_i;
  const double *abs_G, *abs_Om;
  const int *inc_ptr, *inc_ent;
};

__device__ __forceinline__ bool pg_runs(const PgGraph &g, int s) {
  return (g.active == nullptr || g.active[s] != 0) && g.status[s] == 0;
}
__device__ __forceinline__ size_t pg_pose_at(const PgGraph &g, int s, int v) { return ((size_t)v * g.S + s) * 16; }
__device__ __forceinline__ bool pg_free(const PgGraph &g, int v) { return v >= 1 || g.fix_first == 0; }

// ---- fixed-order sums --------------------------------------------------------------------------------------------------
// Every thread brings the serial sum of its strided elements; inside a wave the 64 values are halved (32, 16, .., 1), then
// the PG_THREADS / 64 = 4 wave results are halved (2, 1).  The result reaches every thread.  `red` holds PG_RED doubles: one
// per wave and the result.
__device__ __forceinline__ double block_sum(double v, double *red) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();                       // the previous result has been read by everyone
  if (lane == 0) red[wave] = v;
  __syncthreads();
  if (wave == 0) {
    double t = lane < PG_THREADS / 64 ? red[lane] : 0.0;
#pragma unroll
    for (int off = PG_THREADS / 128; off >= 1; off >>= 1) t += __shfl_down(t, off, 64);
    if (lane == 0) red[PG_THREADS / 64] = t;
  }
  __syncthreads();
  return red[PG_THREADS / 64];
}
__device__ __forceinline__ double block_max(double v, double *red) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  if (wave == 0) {
    double t = lane < PG_THREADS / 64 ? red[lane] : 0.0;
#pragma unroll
    for (int off = PG_THREADS / 128; off >= 1; off >>= 1) t = fmax(t, __shfl_down(t, off, 64));
    if (lane == 0) red[PG_THREADS / 64] = t;
  }
  __syncthreads();
  return red[PG_THREADS / 64];
}

// ---- one edge ----------------------------------------------------------------------------------------------------------

__device__ __forceinline__ void mat6_mul(const double *a, const double *b, double *c) {          // c = a b
#pragma unroll
  for (int r = 0; r < 6; ++r) {
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      double s = a[r * 6] * b[k];
#pragma unroll
      for (int m = 1; m < 6; ++m) s += a[r * 6 + m] * b[m * 6 + k];
      c[r * 6 + k] = s;
    }
  }
}
__device__ __forceinline__ void mat6_tmul(const double *a, const double *b, double *c) {         // c = a^T b
#pragma unroll
  for (int r = 0; r < 6; ++r) {
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      double s = a[r] * b[k];
#pragma unroll
      for (int m = 1; m < 6; ++m) s += a[m * 6 + r] * b[m * 6 + k];
      c[r * 6 + k] = s;
    }
  }
}
__device__ __forceinline__ void mat6_tvec(const double *a, const double *x, double *y) {         // y = a^T x
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    double s = a[r] * x[0];
#pragma unroll
    for (int m = 1; m < 6; ++m) s += a[m * 6 + r] * x[m];
    y[r] = s;
  }
}
__device__ __forceinline__ void mat6_vec_add(const double *a, const double *x, double *y) {      // y += a x
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    double s = a[r * 6] * x[0];
#pragma unroll
    for (int m = 1; m < 6; ++m) s += a[r * 6 + m] * x[m];
    y[r] += s;
  }
}
__device__ __forceinline__ void mat6_tvec_add(const double *a, const double *x, double *y) {     // y += a^T x
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    double s = a[r] * x[0];
#pragma unroll
    for (int m = 1; m < 6; ++m) s += a[m * 6 + r] * x[m];
    y[r] += s;
  }
}

// One edge id of a stream resolved: its ends, measurement, information (nullptr: an odometry edge) and class bit.
struct PgEdge {
  int vi, vj, cls;
  const double *Zp, *Omp;
  bool absolute;
};
// false where the id is no edge of the stream
__device__ __forceinline__ bool pg_edge_at(const PgGraph &g, int s, int id, PgEdge &ed) {
  ed.Omp = nullptr;
  ed.absolute = false;
  if (id < g.N) {
    if (id < 1 || id >= g.count[s]) return false;
    ed.vi = id - 1; ed.vj = id;
    ed.Zp = g.Zc + pg_pose_at(g, s, id);
    ed.cls = PG_CLASS_CHAIN;
  } else if (id < g.N + g.ML) {
    const int l = id - g.N;
    if (l >= g.nloops[s]) return false;
    ed.vi = g.loop_ij[((size_t)s * g.ML + l) * 2];
    ed.vj = g.loop_ij[((size_t)s * g.ML + l) * 2 + 1];
    ed.Zp = g.loop_Z + ((size_t)s * g.ML + l) * 16;
    ed.Omp = g.loop_Om + ((size_t)s * g.ML + l) * 36;
    ed.cls = PG_CLASS_LOOP;
  } else {
    const int a = id - g.N - g.ML;
    if (a >= g.nabs[s]) return false;
    ed.vi = ed.vj = g.abs_i[(size_t)s * g.MA + a];
    ed.Zp = g.abs_G + ((size_t)s * g.MA + a) * 16;
    ed.Omp = g.abs_Om + ((size_t)s * g.MA + a) * 36;
    ed.absolute = true;
    ed.cls = PG_CLASS_ABSOLUTE;
  }
  return true;
}

// The error of an edge at the poses X: Delta = Z^-1 X_i^-1 X_j, e = (t_Delta, sg q_xyz), Omega e and chi = e^T Omega e.
struct PgError {
  double Om[36], e[6], Oe[6], chi, sg;
  Se3 Z, A, D;
  Quat q;
};
__device__ __forceinline__ void pg_edge_error(const PgGraph &g, const double *__restrict__ X, int s, const PgEdge &ed,
                                              PgError &r) {
  if (ed.Omp != nullptr) {
#pragma unroll
    for (int k = 0; k < 36; ++k) r.Om[k] = ed.Omp[k];
  } else {                                       // an odometry edge: diag(2, 2, 2, 5, 5, 5)
#pragma unroll
    for (int k = 0; k < 36; ++k) r.Om[k] = (k % 7 == 0) ? (k < 21 ? 2.0 : 5.0) : 0.0;
  }
  r.Z = se3_load(ed.Zp);
  const Se3 Xj = se3_load(X + pg_pose_at(g, s, ed.vj));
  r.A = Xj;                                      // absolute: the fixed vertex is G itself and Z = I
  if (!ed.absolute) r.A = se3_mul(se3_rigid_inv(se3_load(X + pg_pose_at(g, s, ed.vi))), Xj);
  r.D = se3_mul(se3_rigid_inv(r.Z), r.A);
  r.q = se3_quat(r.D);
  r.sg = r.q.w < 0.0 ? -1.0 : 1.0;
  r.e[0] = r.D.m[3]; r.e[1] = r.D.m[7]; r.e[2] = r.D.m[11];
  r.e[3] = r.sg * r.q.x; r.e[4] = r.sg * r.q.y; r.e[5] = r.sg * r.q.z;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    double t = r.Om[k * 6] * r.e[0];
#pragma unroll
    for (int m = 1; m < 6; ++m) t += r.Om[k * 6 + m] * r.e[m];
    r.Oe[k] = t;
  }
  double chi = r.e[0] * r.Oe[0];
#pragma unroll
  for (int m = 1; m < 6; ++m) chi += r.e[m] * r.Oe[m];
  r.chi = chi;
}

// The kernel of a launch: kind PG_HUBER .. PG_DCS (PG_ROBUST_NONE: none), its delta, and the mask of edge classes it acts on.
struct PgRobust {
  int kind, mask;
  double delta;
};
// rho and w of an edge of class cls with raw term c: an edge outside the mask keeps rho = c, w = 1
__device__ __forceinline__ void pg_edge_robustify(const PgRobust &rb, int cls, double c, double *rho, double *w) {
  pg_robustify((rb.mask & cls) != 0 ? rb.kind : PG_ROBUST_NONE, rb.delta, c, rho, w);
}
// dst (n doubles) = w times the finished block or gradient src (the one order the model repeats); without a kernel: src
template <bool ROBUST, int n>
__device__ __forceinline__ void pg_put(double *__restrict__ dst, const double *src, double w) {
#pragma unroll
  for (int k = 0; k < n; ++k) dst[k] = ROBUST ? w * src[k] : src[k];
}

// grid (ceil(E / 64), S).  FULL: the whole slot from the poses X; otherwise only the chi2 term, into chi_out (S, E).  ROBUST:
// the chi2 term is rho(c), the blocks and gradients carry the weight w = rho'(c) (first order: no rho'' term), and the full
// form leaves the raw c and w in the slot's spare doubles; the plain form never reads rb and never touches those doubles.
template <bool FULL, bool ROBUST>
__global__ __launch_bounds__(PG_EDGE_THREADS) void pg_linearise_kernel(PgGraph g, const double *__restrict__ X,
                                                                       double *__restrict__ slots,
                                                                       double *__restrict__ chi_out, PgRobust rb) {
  const int s = blockIdx.y;
  if (!pg_runs(g, s)) return;
  const int id = blockIdx.x * PG_EDGE_THREADS + threadIdx.x;
  const int E = g.N + g.ML + g.MA;
  if (id >= E) return;
  PgEdge ed;
  if (!pg_edge_at(g, s, id, ed)) return;
  PgError er;
  pg_edge_error(g, X, s, ed, er);
  double rho = er.chi, w = 1.0;
  if (ROBUST) pg_edge_robustify(rb, ed.cls, er.chi, &rho, &w);
  if (!FULL) {
    chi_out[(size_t)s * E + id] = rho;
    return;
  }
  double *slot = slots + ((size_t)s * E + id) * PG_SLOT;
#pragma unroll
  for (int m = 0; m < 6; ++m) {
    slot[PG_E + m] = er.e[m];
    slot[PG_OE + m] = er.Oe[m];
  }
  slot[PG_CHI] = rho;
  if (ROBUST) {
    slot[PG_RAW] = er.chi;
    slot[PG_W] = w;
  }
  const Se3 &Z = er.Z, &A = er.A, &D = er.D;
  const Quat &q = er.q;
  const double sg = er.sg;
  const double *Om = er.Om, *Oe = er.Oe;
  // d e_q / d nu_j = sg (w I + [v]x), d e_t / d rho_j = R_Delta
  const double v[3] = {q.x, q.y, q.z};
  double Jj[36], Ji[36], T[36], B[36], gr[6];
#pragma unroll
  for (int k = 0; k < 36; ++k) Jj[k] = Ji[k] = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) Jj[r * 6 + c] = D.m[4 * r + c];
  }
  Jj[3 * 6 + 3] = sg * q.w; Jj[3 * 6 + 4] = sg * -v[2]; Jj[3 * 6 + 5] = sg * v[1];
  Jj[4 * 6 + 3] = sg * v[2]; Jj[4 * 6 + 4] = sg * q.w; Jj[4 * 6 + 5] = sg * -v[0];
  Jj[5 * 6 + 3] = sg * -v[1]; Jj[5 * 6 + 4] = sg * v[0]; Jj[5 * 6 + 5] = sg * q.w;
  mat6_mul(Om, Jj, T);
  mat6_tmul(Jj, T, B);
  pg_put<ROBUST, 36>(slot + PG_HJJ, B, w);
  mat6_tvec(Jj, Oe, gr);
  pg_put<ROBUST, 6>(slot + PG_BJ, gr, w);
  if (ed.absolute) return;                       // the i side of an absolute edge is the fixed vertex: never read
  // d e_t / d rho_i = -R_Z^T, d e_t / d nu_i = 2 R_Z^T [t_A]x, d e_q / d nu_i = sg (-w I + [v]x) R_Z^T
  const double ta[3] = {A.m[3], A.m[7], A.m[11]};
  const double tx[9] = {0.0, -ta[2], ta[1], ta[2], 0.0, -ta[0], -ta[1], ta[0], 0.0};
  const double qm[9] = {-q.w, -v[2], v[1], v[2], -q.w, -v[0], -v[1], v[0], -q.w};
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      Ji[r * 6 + c] = -Z.m[4 * c + r];
      Ji[r * 6 + 3 + c] = 2.0 * ((Z.m[r] * tx[c] + Z.m[4 + r] * tx[3 + c]) + Z.m[8 + r] * tx[6 + c]);
      Ji[(3 + r) * 6 + 3 + c] = sg * ((qm[r * 3] * Z.m[4 * c] + qm[r * 3 + 1] * Z.m[4 * c + 1]) + qm[r * 3 + 2] * Z.m[4 * c + 2]);
    }
  }
  mat6_tmul(Ji, T, B);                           // Ji^T (Omega Jj)
  pg_put<ROBUST, 36>(slot + PG_HIJ, B, w);
  mat6_tvec(Ji, Oe, gr);
  pg_put<ROBUST, 6>(slot + PG_BI, gr, w);
  mat6_mul(Om, Ji, T);
  mat6_tmul(Ji, T, B);
  pg_put<ROBUST, 36>(slot + PG_HII, B, w);
}

// The read-out of the weights: grid (ceil((ML + MA) / 64), S), one thread per loop and absolute edge id.  out (S, ML + MA, 2):
// the raw term c and the weight w of the edge at the vertices X as they stand, zeros past nloops / nabs.  It runs for idle
// and frozen streams too; without a kernel (or for a class outside the mask) w = 1.
__global__ __launch_bounds__(PG_EDGE_THREADS) void pg_edge_weights_kernel(PgGraph g, const double *__restrict__ X,
                                                                          double *__restrict__ out, PgRobust rb) {
  const int s = blockIdx.y;
  const int k = blockIdx.x * PG_EDGE_THREADS + threadIdx.x;
  if (k >= g.ML + g.MA) return;
  double c = 0.0, w = 0.0;
  PgEdge ed;
  if (pg_edge_at(g, s, g.N + k, ed)) {
    PgError er;
    pg_edge_error(g, X, s, ed, er);
    double rho;
    pg_edge_robustify(rb, ed.cls, er.chi, &rho, &w);
    c = er.chi;
  }
  double *o = out + ((size_t)s * (g.ML + g.MA) + k) * 2;
  o[0] = c;
  o[1] = w;
}

// ---- per-vertex gathers, in one order everywhere: chain edge v (its j side), chain edge v + 1 (its i side), then the vertex's
// incidence list (entries edge id * 2 + side, side 1 = j) --------------------------------------------------------------------

struct PgIncidence {
  const double *slots;     // the stream's slots
  const int *ent;          // the stream's incidence entries
  int lo, hi;              // the vertex's range of them
  bool prev, next;         // chain edges v and v + 1 exist
};
__device__ __forceinline__ PgIncidence pg_incidence(const PgGraph &g, const double *slots, int s, int v, int n) {
  const int E = g.N + g.ML + g.MA;
  PgIncidence in;
  in.slots = slots + (size_t)s * E * PG_SLOT;
  in.ent = g.inc_ent + (size_t)s * (2 * g.ML + g.MA);
  in.lo = g.inc_ptr[(size_t)s * (g.N + 1) + v];
  in.hi = g.inc_ptr[(size_t)s * (g.N + 1) + v + 1];
  if (g.nloops[s] == 0 && g.nabs[s] == 0) in.hi = in.lo;      // a graph emptied on the device: the host's lists are stale
  in.prev = v >= 1;
  in.next = v + 1 < n;
  return in;
}
// the other end of an incidence entry's edge
__device__ __forceinline__ int pg_other(const PgGraph &g, int s, int ent) {
  const int id = ent >> 1;
  if (id >= g.N + g.ML) return -1;
  return g.loop_ij[((size_t)s * g.ML + (id - g.N)) * 2 + ((ent & 1) ? 0 : 1)];
}

__device__ __forceinline__ void pg_gather_b(const PgIncidence &in, int v, double *b) {
#pragma unroll
  for (int m = 0; m < 6; ++m) b[m] = 0.0;
  if (in.prev) {
#pragma unroll
    for (int m = 0; m < 6; ++m) b[m] += in.slots[(size_t)v * PG_SLOT + PG_BJ + m];
  }
  if (in.next) {
#pragma unroll
    for (int m = 0; m < 6; ++m) b[m] += in.slots[(size_t)(v + 1) * PG_SLOT + PG_BI + m];
  }
  for (int k = in.lo; k < in.hi; ++k) {
    const int ent = in.ent[k];
    const double *sl = in.slots + (size_t)(ent >> 1) * PG_SLOT + ((ent & 1) ? PG_BJ : PG_BI);
#pragma unroll
    for (int m = 0; m < 6; ++m) b[m] += sl[m];
  }
}
__device__ __forceinline__ void pg_gather_diag(const PgIncidence &in, int v, double *d) {
#pragma unroll
  for (int m = 0; m < 36; ++m) d[m] = 0.0;
  if (in.prev) {
#pragma unroll
    for (int m = 0; m < 36; ++m) d[m] += in.slots[(size_t)v * PG_SLOT + PG_HJJ + m];
  }
  if (in.next) {
#pragma unroll
    for (int m = 0; m < 36; ++m) d[m] += in.slots[(size_t)(v + 1) * PG_SLOT + PG_HII + m];
  }
  for (int k = in.lo; k < in.hi; ++k) {
    const int ent = in.ent[k];
    const double *sl = in.slots + (size_t)(ent >> 1) * PG_SLOT + ((ent & 1) ? PG_HJJ : PG_HII);
#pragma unroll
    for (int m = 0; m < 36; ++m) d[m] += sl[m];
  }
}
// y = (H + lambda I) p at vertex v; p (N, 6) of the stream (zero at a fixed vertex).  p is written by other threads of the
// workgroup between two calls, so it is read through a plain pointer after a barrier.
__device__ __forceinline__ void pg_hprod(const PgGraph &g, const PgIncidence &in, int s, int v, double lambda,
                                         const double *p, double *y) {
  const double *pv = p + (size_t)v * 6;
#pragma unroll
  for (int m = 0; m < 6; ++m) y[m] = lambda * pv[m];
  if (in.prev) {
    const double *sl = in.slots + (size_t)v * PG_SLOT;
    mat6_vec_add(sl + PG_HJJ, pv, y);
    mat6_tvec_add(sl + PG_HIJ, pv - 6, y);
  }
  if (in.next) {
    const double *sl = in.slots + (size_t)(v + 1) * PG_SLOT;
    mat6_vec_add(sl + PG_HII, pv, y);
    mat6_vec_add(sl + PG_HIJ, pv + 6, y);
  }
  for (int k = in.lo; k < in.hi; ++k) {
    const int ent = in.ent[k];
    const double *sl = in.slots + (size_t)(ent >> 1) * PG_SLOT;
    const int o = pg_other(g, s, ent);
    if (ent & 1) {
      mat6_vec_add(sl + PG_HJJ, pv, y);
      if (o >= 0) mat6_tvec_add(sl + PG_HIJ, p + (size_t)o * 6, y);
    } else {
      mat6_vec_add(sl + PG_HII, pv, y);
      mat6_vec_add(sl + PG_HIJ, p + (size_t)o * 6, y);
    }
  }
}

// In-place inverse of a symmetric positive definite 6 x 6 matrix (Gauss-Jordan, no pivoting).
__device__ __forceinline__ void mat6_invert(double *a) {
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const double pv = 1.0 / a[k * 6 + k];
    a[k * 6 + k] = 1.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) a[k * 6 + c] *= pv;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      if (r == k) continue;
      const double f = a[r * 6 + k];
      a[r * 6 + k] = 0.0;
#pragma unroll
      for (int c = 0; c < 6; ++c) a[r * 6 + c] -= f * a[k * 6 + c];
    }
  }
}

// ---- solve -------------------------------------------------------------------------------------------------------------
// grid (S), PG_THREADS threads; thread t owns the vertices t, t + PG_THREADS, ...
__global__ __launch_bounds__(PG_THREADS) void pg_solve_kernel(PgGraph g, int it, int pcg_iters, double pcg_tol,
                                                              int *status, const double *__restrict__ slots,
                                                              const double *__restrict__ X, double *work, double *delta,
                                                              double *__restrict__ Xt, double *lam, double *nu, double *chi2,
                                                              int *__restrict__ pcg_used, double *__restrict__ relres,
                                                              int diag_stride) {
  __shared__ double red[PG_RED];
  const int s = blockIdx.x;
  if (!pg_runs(g, s)) return;
  const int n = g.count[s], E = g.N + g.ML + g.MA, tid = threadIdx.x;
  const size_t sec = (size_t)g.S * g.N * 6, at = (size_t)s * g.N * 6;
  double *r = work + PG_W_R * sec + at, *z = work + PG_W_Z * sec + at, *p = work + PG_W_P * sec + at,
         *Ap = work + PG_W_AP * sec + at, *gb = work + PG_W_G * sec + at,
         *Minv = work + PG_W_MINV * sec + (size_t)s * g.N * 36, *x = delta + at;
  const double *sl = slots + (size_t)s * E * PG_SLOT;

  // chi2 of the linearisation point, over every edge id in order (ids that are no edge bring zero)
  double acc = 0.0;
  for (int id = tid; id < E; id += PG_THREADS) {
    const bool edge = id < g.N ? (id >= 1 && id < n) : id < g.N + g.ML ? id - g.N < g.nloops[s]
                                                                        : id - g.N - g.ML < g.nabs[s];
    acc += edge ? sl[(size_t)id * PG_SLOT + PG_CHI] : 0.0;
  }
  const double chi = block_sum(acc, red);
  if (!(fabs(chi) <= 1.79769313486231570815e308)) {           // NaN or Inf: some pose, measurement or information is not finite
    if (tid == 0) status[s] = PG_NONFINITE;
    return;
  }
  // the gradient and the block diagonal per vertex
  double dmax = 0.0, bmax = 0.0, bb = 0.0;
  for (int v = tid; v < n; v += PG_THREADS) {
    double b[6], d[36];
#pragma unroll
    for (int m = 0; m < 6; ++m) x[(size_t)v * 6 + m] = 0.0;
    if (!pg_free(g, v)) {
#pragma unroll
      for (int m = 0; m < 6; ++m) {
        gb[(size_t)v * 6 + m] = 0.0; r[(size_t)v * 6 + m] = 0.0; z[(size_t)v * 6 + m] = 0.0; p[(size_t)v * 6 + m] = 0.0;
      }
      continue;
    }
    const PgIncidence in = pg_incidence(g, slots, s, v, n);
    pg_gather_b(in, v, b);
    pg_gather_diag(in, v, d);
#pragma unroll
    for (int m = 0; m < 6; ++m) {
      gb[(size_t)v * 6 + m] = b[m];
      bmax = fmax(bmax, fabs(b[m]));
      dmax = fmax(dmax, d[m * 7]);
      bb += b[m] * b[m];
    }
#pragma unroll
    for (int m = 0; m < 36; ++m) Minv[(size_t)v * 36 + m] = d[m];
  }
  dmax = block_max(dmax, red);
  bmax = block_max(bmax, red);
  const double bnorm = sqrt(block_sum(bb, red));
  double lambda = lam[s];
  if (it == 0) lambda = 1e-5 * dmax;
  if (tid == 0) {
    chi2[s] = chi;
    if (it == 0) {
      lam[s] = lambda;
      nu[s] = 2.0;
    }
  }
  if (bmax <= 1e-12) {                                         // a stationary point
    if (tid == 0) status[s] = PG_CONVERGED;
    return;
  }
  // r = -b, z = M^-1 r, p = z
  double rz_l = 0.0;
  for (int v = tid; v < n; v += PG_THREADS) {
    if (!pg_free(g, v)) continue;
    double d[36];
#pragma unroll
    for (int m = 0; m < 36; ++m) d[m] = Minv[(size_t)v * 36 + m];
#pragma unroll
    for (int m = 0; m < 6; ++m) d[m * 7] += lambda;
    mat6_invert(d);
    double rv[6], zv[6];
#pragma unroll
    for (int m = 0; m < 6; ++m) {
      rv[m] = -gb[(size_t)v * 6 + m];
      zv[m] = 0.0;
    }
    mat6_vec_add(d, rv, zv);
#pragma unroll
    for (int m = 0; m < 36; ++m) Minv[(size_t)v * 36 + m] = d[m];
#pragma unroll
    for (int m = 0; m < 6; ++m) {
      r[(size_t)v * 6 + m] = rv[m]; z[(size_t)v * 6 + m] = zv[m]; p[(size_t)v * 6 + m] = zv[m];
      rz_l += rv[m] * zv[m];
    }
  }
  double rz = block_sum(rz_l, red);                            // (its barriers also publish p)
  double rr = bnorm * bnorm;
  int used = 0;
  for (int k = 0; k < pcg_iters; ++k) {
    double pAp_l = 0.0;
    for (int v = tid; v < n; v += PG_THREADS) {
      if (!pg_free(g, v)) continue;
      const PgIncidence in = pg_incidence(g, slots, s, v, n);
      double y[6];
      pg_hprod(g, in, s, v, lambda, p, y);
#pragma unroll
      for (int m = 0; m < 6; ++m) {
        Ap[(size_t)v * 6 + m] = y[m];
        pAp_l += p[(size_t)v * 6 + m] * y[m];
      }
    }
    const double pAp = block_sum(pAp_l, red);
    if (!(pAp > 0.0)) break;                                   // not positive definite in floating point: keep x
    const double alpha = rz / pAp;
    double rz_n = 0.0, rr_n = 0.0;
    for (int v = tid; v < n; v += PG_THREADS) {
      if (!pg_free(g, v)) continue;
      double rv[6], zv[6];
#pragma unroll
      for (int m = 0; m < 6; ++m) {
        x[(size_t)v * 6 + m] += alpha * p[(size_t)v * 6 + m];
        rv[m] = r[(size_t)v * 6 + m] - alpha * Ap[(size_t)v * 6 + m];
        r[(size_t)v * 6 + m] = rv[m];
        zv[m] = 0.0;
      }
      mat6_vec_add(Minv + (size_t)v * 36, rv, zv);
#pragma unroll
      for (int m = 0; m < 6; ++m) {
        z[(size_t)v * 6 + m] = zv[m];
        rz_n += rv[m] * zv[m];
        rr_n += rv[m] * rv[m];
      }
    }
    rz_n = block_sum(rz_n, red);
    rr = block_sum(rr_n, red);
    used = k + 1;
    if (sqrt(rr) <= pcg_tol * bnorm) break;
    const double beta = rz_n / rz;
    rz = rz_n;
    for (int v = tid; v < n; v += PG_THREADS) {
      if (!pg_free(g, v)) continue;
#pragma unroll
      for (int m = 0; m < 6; ++m) p[(size_t)v * 6 + m] = z[(size_t)v * 6 + m] + beta * p[(size_t)v * 6 + m];
    }
    __syncthreads();                                           // p is read across vertices next
  }
  if (tid == 0) {
    pcg_used[(size_t)s * diag_stride + it] = used;
    relres[(size_t)s * diag_stride + it] = sqrt(rr) / bnorm;
  }
  // the trial poses
  for (int v = tid; v < n; v += PG_THREADS) {
    const Se3 xv = se3_load(X + pg_pose_at(g, s, v));
    se3_store(Xt + pg_pose_at(g, s, v), pg_free(g, v) ? pg_retract(xv, x + (size_t)v * 6) : xv);
  }
}

// The retraction alone: Xt[v] = X[v] . D(delta[v]) for the vertices in use of the running streams (a fixed vertex is copied).
__global__ __launch_bounds__(PG_THREADS) void pg_retract_kernel(PgGraph g, const double *__restrict__ X,
                                                                const double *__restrict__ delta, double *__restrict__ Xt) {
  const int s = blockIdx.x;
  if (!pg_runs(g, s)) return;
  const int n = g.count[s];
  for (int v = threadIdx.x; v < n; v += PG_THREADS) {
    const Se3 xv = se3_load(X + pg_pose_at(g, s, v));
    se3_store(Xt + pg_pose_at(g, s, v), pg_free(g, v) ? pg_retract(xv, delta + ((size_t)s * g.N + v) * 6) : xv);
  }
}

// ---- judge -------------------------------------------------------------------------------------------------------------
// grid (S), PG_THREADS threads.  chi_new (S, E): the chi2 terms at the trial poses.
__global__ __launch_bounds__(PG_THREADS) void pg_judge_kernel(PgGraph g, int it, int *status, const double *__restrict__ slots,
                                                              const double *__restrict__ chi_new,
                                                              const double *__restrict__ delta, const double *__restrict__ Xt,
                                                              double *__restrict__ X, double *lam, double *nu, double *chi2,
                                                              int *__restrict__ accepted, int diag_stride) {
  __shared__ double red[PG_RED];
  __shared__ int take;
  const int s = blockIdx.x;
  if (!pg_runs(g, s)) return;
  const int n = g.count[s], E = g.N + g.ML + g.MA, tid = threadIdx.x;
  const double lambda = lam[s];
  double acc = 0.0;
  for (int id = tid; id < E; id += PG_THREADS) {
    const bool edge = id < g.N ? (id >= 1 && id < n) : id < g.N + g.ML ? id - g.N < g.nloops[s]
                                                                        : id - g.N - g.ML < g.nabs[s];
    acc += edge ? chi_new[(size_t)s * E + id] : 0.0;
  }
  const double chi_n = block_sum(acc, red);
  // delta^T (lambda delta - b)
  acc = 0.0;
  for (int v = tid; v < n; v += PG_THREADS) {
    if (!pg_free(g, v)) continue;
    double b[6];
    pg_gather_b(pg_incidence(g, slots, s, v, n), v, b);
    const double *d = delta + ((size_t)s * g.N + v) * 6;
    double t = d[0] * (lambda * d[0] - b[0]);
#pragma unroll
    for (int m = 1; m < 6; ++m) t += d[m] * (lambda * d[m] - b[m]);
    acc += t;
  }
  const double scale = block_sum(acc, red);
  if (tid == 0) {
    const double chi = chi2[s];
    const double rho = (chi - chi_n) / scale;
    const bool ok = rho > 0.0 && fabs(chi_n) <= 1.79769313486231570815e308;
    if (ok) {
      const double t = 2.0 * rho - 1.0;
      const double a = 1.0 - (t * t) * t;
      lam[s] = lambda * fmax(1.0 / 3.0, a);
      nu[s] = 2.0;
      if (chi - chi_n <= 1e-9 * chi) status[s] = PG_CONVERGED;
      chi2[s] = chi_n;
    } else {
      const double m = nu[s];
      lam[s] = lambda * m;
      nu[s] = 2.0 * m;
    }
    accepted[(size_t)s * diag_stride + it] = ok ? 1 : 0;
    take = ok ? 1 : 0;
  }
  __syncthreads();
  if (take == 0) return;
  for (int k = tid; k < n * 16; k += PG_THREADS) {
    const size_t a = pg_pose_at(g, s, k >> 4) + (k & 15);
    X[a] = Xt[a];
  }
}

// ---- begin and append: one thread per stream -----------------------------------------------------------------------------

// The first launch of an optimisation: an active stream gets status 0, or CONVERGED | TRIVIAL where its graph is a chain
// without loop or absolute edges (chi2 = 0 already: nothing may move); the diagnostics rows of the call are cleared.
__global__ __launch_bounds__(1024) void pg_begin_kernel(int S, int iters, int diag_stride, const int *__restrict__ active,
                                                        const int *__restrict__ count, const int *__restrict__ nloops,
                                                        const int *__restrict__ nabs, int *__restrict__ status,
                                                        int *__restrict__ pcg_used, double *__restrict__ relres,
                                                        int *__restrict__ accepted, double *__restrict__ chi2) {
  const int s = threadIdx.x;
  if (s >= S || (active != nullptr && active[s] == 0)) return;
  const bool trivial = count[s] <= 1 || (nloops[s] == 0 && nabs[s] == 0);
  status[s] = trivial ? (PG_CONVERGED | PG_TRIVIAL) : 0;
  if (trivial) chi2[s] = 0.0;
  for (int k = 0; k < iters; ++k) {
    pcg_used[(size_t)s * diag_stride + k] = 0;
    relres[(size_t)s * diag_stride + k] = 0.0;
    accepted[(size_t)s * diag_stride + k] = 0;
  }
}

// rel (S, 4, 4) fp64, or rows (S, 7) fp32 [tx ty tz qw qx qy qz].  Pair (active and valid): k = count (with the stream
// engine's words, stream_count given: k = stream_count - 1, the row its append just wrote, which must be the graph's next
// vertex), X[k] = X[k-1] . Z, Zc[k] = Z, count = k + 1; k >= N, or a k that is not the next vertex, sets *overflow and writes
// nothing.  Prime (active and not valid): an empty graph -- count = 1, X[0] = I, no loop and no absolute edge, epoch + 1 (the
// host drops its edge lists when it sees the epoch move).
__global__ __launch_bounds__(1024) void pg_append_kernel(int S, int N, const int *__restrict__ active,
                                                         const int *__restrict__ valid,
                                                         const int *__restrict__ stream_count,
                                                         const double *__restrict__ rel,
                                                         const float *__restrict__ rows, double *__restrict__ X,
                                                         double *__restrict__ Zc, int *__restrict__ count,
                                                         int *__restrict__ nloops, int *__restrict__ nabs,
                                                         int *__restrict__ epoch, int *__restrict__ overflow) {
  const int s = threadIdx.x;
  if (s >= S || (active != nullptr && active[s] == 0)) return;
  if (valid == nullptr || valid[s] != 0) {
    const int k = stream_count != nullptr ? stream_count[s] - 1 : count[s];
    if (k < 1 || k >= N || k != count[s]) {
      *overflow = 1;
      return;
    }
    const Se3 z = rel != nullptr ? se3_load(rel + (size_t)s * 16) : pose_row_to_se3(rows + (size_t)s * 7);
    const size_t at = ((size_t)k * S + s) * 16;
    se3_store(Zc + at, z);
    se3_store(X + at, se3_mul(se3_load(X + at - (size_t)S * 16), z));
    count[s] = k + 1;
    return;
  }
  const Se3 id = se3_identity();
  se3_store(X + (size_t)s * 16, id);
  se3_store(Zc + (size_t)s * 16, id);
  count[s] = 1;
  nloops[s] = 0;
  nabs[s] = 0;
  epoch[s] += 1;
}

}  // namespace pwclo

using namespace pwclo;

// `measured`: the launch reads the measurements (Zc, loop_Z, loop_Om, abs_G, abs_Om); otherwise they may be null.
static bool pg_graph(PgGraph &g, const char *what, bool measured, int S, int N, int ML, int MA, int fix_first, const int *active,
                     const int *status, const int *count, const int *nloops, const int *nabs, const double *Zc,
                     const int *loop_ij, const double *loop_Z, const double *loop_Om, const int *abs_i, const double *abs_G,
                     const double *abs_Om, const int *inc_ptr, const int *inc_ent) {
  if (!(S >= 1 && S <= PG_MAX_STREAMS)) {
    set_error(PWCLO_EINVAL, "%s: S=%d streams outside [1, %d]", what, S, PG_MAX_STREAMS);
    return false;
  }
  if (!(N >= 1 && ML >= 1 && MA >= 1) || (long long)N + ML + MA > (1 << 24)) {
    set_error(PWCLO_EINVAL, "%s: capacities max_poses=%d max_loops=%d max_absolute=%d must be >= 1 and sum to at most 2^24",
              what, N, ML, MA);
    return false;
  }
  if (!(status && count && nloops && nabs && loop_ij && abs_i) ||
      (measured && !(Zc && loop_Z && loop_Om && abs_G && abs_Om))) {
    set_error(PWCLO_EINVAL, "%s: a null argument", what);
    return false;
  }
  g = PgGraph{S, N, ML, MA, fix_first, active, status, count, nloops, nabs, Zc, loop_ij, loop_Z, loop_Om, abs_i, abs_G,
              abs_Om, inc_ptr, inc_ent};
  return true;
}

extern "C" void pose_graph_begin_kernel_wrapper(int S, int iters, int diag_stride, const int *active, const int *count,
                                                const int *nloops, const int *nabs, int *status, int *pcg_used,
                                                double *relres, int *accepted, double *chi2) {
  PWCLO_REQUIRE(S >= 1 && S <= PG_MAX_STREAMS, "pose_graph_begin: S=%d streams outside [1, %d]", S, PG_MAX_STREAMS);
  PWCLO_REQUIRE(iters >= 1 && iters <= diag_stride, "pose_graph_begin: iters=%d outside [1, diag_stride=%d]", iters,
                diag_stride);
  PWCLO_REQUIRE(count && nloops && nabs && status && pcg_used && relres && accepted && chi2,
                "pose_graph_begin: a null argument");
  hipLaunchKernelGGL(pg_begin_kernel, dim3(1), dim3(ceil_div(S, 64) * 64), 0, current_stream(), S, iters, diag_stride, active,
                     count, nloops, nabs, status, pcg_used, relres, accepted, chi2);
  check_launch("pose_graph_begin");
}

extern "C" void pose_graph_append_kernel_wrapper(int S, int N, const int *active, const int *valid,
                                                 const int *stream_count, const double *rel, const float *rows, double *X, double *Zc, int *count, int *nloops, int *nabs,
                                                 int *epoch, int *overflow) {
  PWCLO_REQUIRE(S >= 1 && S <= PG_MAX_STREAMS, "pose_graph_append: S=%d streams outside [1, %d]", S, PG_MAX_STREAMS);
  PWCLO_REQUIRE(N >= 1, "pose_graph_append: max_poses=%d must be >= 1", N);
  PWCLO_REQUIRE((rel != nullptr) != (rows != nullptr), "pose_graph_append: exactly one of rel and rows is given");
  PWCLO_REQUIRE(X && Zc && count && nloops && nabs && epoch && overflow, "pose_graph_append: a null argument");
  hipLaunchKernelGGL(pg_append_kernel, dim3(1), dim3(ceil_div(S, 64) * 64), 0, current_stream(), S, N, active, valid,
                     stream_count, rel, rows, X, Zc, count, nloops, nabs, epoch, overflow);
  check_launch("pose_graph_append");
}

extern "C" void pose_graph_linearise_kernel_wrapper(int S, int N, int ML, int MA, const int *active, const int *status,
                                                    const int *count, const int *nloops, const int *nabs, const double *X,
                                                    const double *Zc, const int *loop_ij, const double *loop_Z,
                                                    const double *loop_Om, const int *abs_i, const double *abs_G,
                                                    const double *abs_Om, double *slots, double *chi_only) {
  PgGraph g;
  if (!pg_graph(g, "pose_graph_linearise", true, S, N, ML, MA, 1, active, status, count, nloops, nabs, Zc, loop_ij, loop_Z, loop_Om,
                abs_i, abs_G, abs_Om, nullptr, nullptr))
    return;
  PWCLO_REQUIRE(X && (slots != nullptr) != (chi_only != nullptr),
                "pose_graph_linearise: X and exactly one of slots and chi_only are needed");
  const dim3 grid(ceil_div(N + ML + MA, PG_EDGE_THREADS), S);
  const PgRobust none{PG_ROBUST_NONE, 0, 0.0};
  if (slots != nullptr)
    hipLaunchKernelGGL((pg_linearise_kernel<true, false>), grid, dim3(PG_EDGE_THREADS), 0, current_stream(), g, X, slots,
                       chi_only, none);
  else
    hipLaunchKernelGGL((pg_linearise_kernel<false, false>), grid, dim3(PG_EDGE_THREADS), 0, current_stream(), g, X, slots,
                       chi_only, none);
  check_launch("pose_graph_linearise");
}

// kind 0 (no kernel) is accepted only where `optional`; a kernel needs a finite delta > 0 and a mask of at least one class
static bool pg_robust(PgRobust &rb, const char *what, bool optional, int kind, int edge_mask, double delta) {
  if (!(kind >= (optional ? PG_ROBUST_NONE : PG_HUBER) && kind <= PG_DCS)) {
    set_error(PWCLO_EINVAL, "%s: kernel kind %d outside [%d, %d]", what, kind, optional ? PG_ROBUST_NONE : PG_HUBER, PG_DCS);
    return false;
  }
  const int all = PG_CLASS_CHAIN | PG_CLASS_LOOP | PG_CLASS_ABSOLUTE;
  if (kind != PG_ROBUST_NONE && !(edge_mask >= 1 && edge_mask <= all)) {
    set_error(PWCLO_EINVAL, "%s: edge_mask=%d outside [1, %d]", what, edge_mask, all);
    return false;
  }
  if (kind != PG_ROBUST_NONE && !(delta > 0.0 && delta <= 1.79769313486231570815e308)) {
    set_error(PWCLO_EINVAL, "%s: delta=%g must be finite and > 0", what, delta);
    return false;
  }
  rb = kind == PG_ROBUST_NONE ? PgRobust{PG_ROBUST_NONE, 0, 0.0} : PgRobust{kind, edge_mask, delta};
  return true;
}

extern "C" void pose_graph_linearise_robust_kernel_wrapper(int S, int N, int ML, int MA, int kind, int edge_mask, double delta,
                                                           const int *active, const int *status, const int *count,
                                                           const int *nloops, const int *nabs, const double *X,
                                                           const double *Zc, const int *loop_ij, const double *loop_Z,
                                                           const double *loop_Om, const int *abs_i, const double *abs_G,
                                                           const double *abs_Om, double *slots, double *chi_only) {
  PgGraph g;
  PgRobust rb;
  if (!pg_graph(g, "pose_graph_linearise_robust", true, S, N, ML, MA, 1, active, status, count, nloops, nabs, Zc, loop_ij,
                loop_Z, loop_Om, abs_i, abs_G, abs_Om, nullptr, nullptr) ||
      !pg_robust(rb, "pose_graph_linearise_robust", false, kind, edge_mask, delta))
    return;
  PWCLO_REQUIRE(X && (slots != nullptr) != (chi_only != nullptr),
                "pose_graph_linearise_robust: X and exactly one of slots and chi_only are needed");
  const dim3 grid(ceil_div(N + ML + MA, PG_EDGE_THREADS), S);
  if (slots != nullptr)
    hipLaunchKernelGGL((pg_linearise_kernel<true, true>), grid, dim3(PG_EDGE_THREADS), 0, current_stream(), g, X, slots,
                       chi_only, rb);
  else
    hipLaunchKernelGGL((pg_linearise_kernel<false, true>), grid, dim3(PG_EDGE_THREADS), 0, current_stream(), g, X, slots,
                       chi_only, rb);
  check_launch("pose_graph_linearise_robust");
}

extern "C" void pose_graph_edge_weights_kernel_wrapper(int S, int N, int ML, int MA, int kind, int edge_mask, double delta,
                                                       const int *nloops, const int *nabs, const double *X,
                                                       const int *loop_ij, const double *loop_Z, const double *loop_Om,
                                                       const int *abs_i, const double *abs_G, const double *abs_Om,
                                                       double *out) {
  PgGraph g;
  PgRobust rb;
  const int *unread = nloops;                    // status and count: a read-out runs whatever they say, and reads no chain edge
  const double *none = nullptr;
  if (!pg_graph(g, "pose_graph_edge_weights", false, S, N, ML, MA, 1, nullptr, unread, unread, nloops, nabs, none, loop_ij,
                loop_Z, loop_Om, abs_i, abs_G, abs_Om, nullptr, nullptr) ||
      !pg_robust(rb, "pose_graph_edge_weights", true, kind, edge_mask, delta))
    return;
  PWCLO_REQUIRE(X && out && loop_Z && loop_Om && abs_G && abs_Om, "pose_graph_edge_weights: a null argument");
  hipLaunchKernelGGL(pg_edge_weights_kernel, dim3(ceil_div(ML + MA, PG_EDGE_THREADS), S), dim3(PG_EDGE_THREADS), 0,
                     current_stream(), g, X, out, rb);
  check_launch("pose_graph_edge_weights");
}

extern "C" void pose_graph_solve_kernel_wrapper(int S, int N, int ML, int MA, int fix_first, int it, int pcg_iters,
                                                double pcg_tol, const int *active, int *status, const int *count,
                                                const int *nloops, const int *nabs, const int *loop_ij, const int *abs_i,
                                                const int *inc_ptr, const int *inc_ent, const double *slots, const double *X,
                                                double *work, double *delta, double *Xt, double *lam, double *nu,
                                                double *chi2, int *pcg_used, double *relres, int diag_stride) {
  PgGraph g;
  const double *none = nullptr;                  // the measurements are not read here
  if (!pg_graph(g, "pose_graph_solve", false, S, N, ML, MA, fix_first, active, status, count, nloops, nabs, none, loop_ij, none, none,
                abs_i, none, none, inc_ptr, inc_ent))
    return;
  PWCLO_REQUIRE(pcg_iters >= 1 && pcg_tol >= 0.0 && pcg_tol < 1.0, "pose_graph_solve: pcg_iters=%d must be >= 1 and pcg_tol=%g in [0, 1)",
                pcg_iters, pcg_tol);
  PWCLO_REQUIRE(it >= 0 && it < diag_stride, "pose_graph_solve: it=%d outside [0, diag_stride=%d)", it, diag_stride);
  PWCLO_REQUIRE(inc_ptr && inc_ent && slots && X && work && delta && Xt && lam && nu && chi2 && pcg_used && relres,
                "pose_graph_solve: a null argument");
  hipLaunchKernelGGL(pg_solve_kernel, dim3(S), dim3(PG_THREADS), 0, current_stream(), g, it, pcg_iters, pcg_tol, status, slots,
                     X, work, delta, Xt, lam, nu, chi2, pcg_used, relres, diag_stride);
  check_launch("pose_graph_solve");
}

extern "C" void pose_graph_retract_kernel_wrapper(int S, int N, int fix_first, const int *active, const int *status,
                                                  const int *count, const double *X, const double *delta, double *Xt) {
  PWCLO_REQUIRE(S >= 1 && S <= PG_MAX_STREAMS, "pose_graph_retract: S=%d streams outside [1, %d]", S, PG_MAX_STREAMS);
  PWCLO_REQUIRE(N >= 1, "pose_graph_retract: max_poses=%d must be >= 1", N);
  PWCLO_REQUIRE(status && count && X && delta && Xt, "pose_graph_retract: a null argument");
  PgGraph g{S, N, 1, 1, fix_first, active, status, count, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
            nullptr, nullptr, nullptr, nullptr};
  hipLaunchKernelGGL(pg_retract_kernel, dim3(S), dim3(PG_THREADS), 0, current_stream(), g, X, delta, Xt);
  check_launch("pose_graph_retract");
}

extern "C" void pose_graph_judge_kernel_wrapper(int S, int N, int ML, int MA, int fix_first, int it, const int *active,
                                                int *status, const int *count, const int *nloops, const int *nabs,
                                                const int *loop_ij, const int *abs_i, const int *inc_ptr, const int *inc_ent,
                                                const double *slots, const double *chi_new, const double *delta,
                                                const double *Xt, double *X, double *lam, double *nu, double *chi2,
                                                int *accepted, int diag_stride) {
  PgGraph g;
  const double *none = nullptr;
  if (!pg_graph(g, "pose_graph_judge", false, S, N, ML, MA, fix_first, active, status, count, nloops, nabs, none, loop_ij, none, none,
                abs_i, none, none, inc_ptr, inc_ent))
    return;
  PWCLO_REQUIRE(it >= 0 && it < diag_stride, "pose_graph_judge: it=%d outside [0, diag_stride=%d)", it, diag_stride);
  PWCLO_REQUIRE(inc_ptr && inc_ent && slots && chi_new && delta && Xt && X && lam && nu && chi2 && accepted,
                "pose_graph_judge: a null argument");
  hipLaunchKernelGGL(pg_judge_kernel, dim3(S), dim3(PG_THREADS), 0, current_stream(), g, it, status, slots, chi_new, delta, Xt,
                     X, lam, nu, chi2, accepted, diag_stride);
  check_launch("pose_graph_judge");
}
