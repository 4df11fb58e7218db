// Projected GLTR (Gould, Lucidi, Roma & Toint 1999; ipsolver/gltr.py): the Lanczos recurrence on
// the projected Hessian, the trust-region problem of its tridiagonal T solved exactly on the
// device after every step, and the recombination x = x0 + Q h.
//
// State block (ipx_gltr_state_doubles(kmax)):
//     [0] stop code (0 running, 4 tolerance / invariant subspace, 1 cap)   [1] vectors used k
//     [2] gamma_0  [3] R  [4] tol  [5] lambda  [6] ||h||  [7] q_T(h)  [8] gamma_{k+1}
//     [9] case (0 interior, 1 boundary, 2 near-hard)  [10] cap on k  [11] exit path of the solve
//     [12] its rounds  [13] delta_{k-1}  [14..15] spare
//     [16 ...] diag[kmax] (delta_j), off[kmax] (gamma_{j+1}), h[kmax]
//
// One step from w = Z H q_k is four launches, every one of them behind the stop word:
//   k_gltr_delta (grid)    partials of delta = q_k'w
//   k_gltr_update (grid)   every workgroup folds them in the same order; column k + 1 of Q
//                          <- w - delta q_k - gamma_k q_{k-1}, partials of its squared norm
//   k_gltr_solve (one wg)  folds both, appends to T, solves the tridiagonal problem, decides,
//                          writes the header and h
//   k_gltr_next (grid)     column k + 1 of Q /= gamma_{k+1}
//
// The tridiagonal solve (gltr_tridiag) is one __host__ __device__ routine written over "lanes":
// on the device lane t is thread t of the one workgroup, on the host (ipx_gltr_tridiag_host) the
// lanes of a phase run one after the other, so both do the same operations on the same numbers.
//   * interior check: lane 0 factors T = U D U' from the bottom up and solves T h = -gamma_0 e_1
//     (two sweeps of k; all that the steps before the boundary pay);
//   * lambda_min(T): multisection by Sturm counts, 256 shifts per round (one per lane);
//   * the secular equation ||h(lambda)|| = R: 64 shifts per round (one wave; lane t keeps its
//     h(lambda_t) in a column of LDS), geometrically spaced right of the pole, one of them the
//     Newton iterate of 1/||h|| - 1/R from the left end of the bracket; the bracket shrinks to
//     the two shifts around the root, so a round is worth a Newton step AND a 64-section;
//   * near-hard case / collapsed bracket: the step to the boundary along the lowest
//     eigenvector (inverse iteration, lane 0).
#include "ipx_common.h"
#include <float.h>
#include <math.h>
#include <string.h>
#include <vector>

#define GLTR_HDR 16
#define GLTR_MAXV IPX_GLTR_MAX_VECTORS
#define GLTR_NT IPX_BLOCK        // lanes (shifts of a Sturm round)
#define GLTR_NS 64               // shifts of a secular round
#define GLTR_MAX_ROUNDS 40
#define GLTR_EPS 2.220446049250313e-16     // 2^-52

namespace {

struct GltrShared {
  double d[GLTR_MAXV], o[GLTR_MAXV];       // T
  double h[GLTR_MAXV], u[GLTR_MAXV], e[GLTR_MAXV];
  double lam[GLTR_NS], nn[GLTR_NS], w3[GLTR_NS];
  int pd[GLTR_NS];
  int cnt[GLTR_NT];
  double a, b, p, tmax, lamL, lo, hi, newt, sa, sb, rt;
  int geo, has_newt, sel, done, path, rounds, pd0;
};

#ifdef __HIP_DEVICE_COMPILE__
#define GLTR_SYNC() __syncthreads()
#define GLTR_LANES(t, N) for (int t = tid; t < (N); t += GLTR_NT)
#define GLTR_LANE0 (tid == 0)
#else
#define GLTR_SYNC() do { } while (0)
#define GLTR_LANES(t, N) for (int t = 0; t < (N); ++t)
#define GLTR_LANE0 true
#endif

// h(lam) = -(T + lam I)^-1 g0 e_1 into col[i * stride], with T + lam I = U D U' factored from
// the bottom up (pivots e_i = d_i + lam - o_i^2 / e_{i+1}) so that h is one forward recurrence.
// pd: every pivot > 0; nn = ||h||^2; w3 = h'(T + lam I)^-1 h (want3; a third sweep that forms
// the pivots again in the same operations instead of storing them).
__host__ __device__ inline void gltr_eval(int k, const double *d, const double *o, double g0,
                                          double lam, double *col, int stride, int want3,
                                          int &pd, double &nn, double &w3) {
  pd = 1;
  nn = HUGE_VAL;
  w3 = 0.0;
  double e = d[k - 1] + lam;
  col[(k - 1) * stride] = e;
  if (!(e > 0.0)) pd = 0;
  for (int i = k - 2; i >= 0; --i) {
    e = (d[i] + lam) - (o[i] * o[i]) / e;
    col[i * stride] = e;
    if (!(e > 0.0)) pd = 0;
  }
  if (!pd) return;
  double x = -g0 / col[0];
  double s = x * x;
  col[0] = x;
  for (int i = 1; i < k; ++i) {
    x = -(o[i - 1] * x) / col[i * stride];
    col[i * stride] = x;
    s += x * x;
  }
  nn = s;
  if (!want3) return;
  e = d[k - 1] + lam;
  double z = col[(k - 1) * stride];
  double acc = (z * z) / e;
  for (int i = k - 2; i >= 0; --i) {
    z = col[i * stride] - (o[i] / e) * z;
    e = (d[i] + lam) - (o[i] * o[i]) / e;
    acc += (z * z) / e;
  }
  w3 = acc;
}

// eigenvalues of T below sigma
__host__ __device__ inline int gltr_sturm(int k, const double *d, const double *o, double sigma,
                                          double pivmin) {
  int c = 0;
  double q = d[0] - sigma;
  if (fabs(q) <= pivmin) q = -pivmin;
  if (q < 0.0) ++c;
  for (int i = 1; i < k; ++i) {
    q = (d[i] - sigma) - (o[i - 1] * o[i - 1]) / q;
    if (fabs(q) <= pivmin) q = -pivmin;
    if (q < 0.0) ++c;
  }
  return c;
}

// lane 0: S.h <- S.h + tau u, u the lowest eigenvector of T (four inverse iterations at the
// shift mu, just right of -lambda_min), tau the root of ||h + tau u|| = R with the lower model
__host__ __device__ inline void gltr_eig_step(GltrShared &S, int k, double g0, double R,
                                              double mu) {
  const double *d = S.d, *o = S.o;
  const double floor_ = S.tmax > 0.0 ? GLTR_EPS * S.tmax : DBL_MIN;
  double e = d[k - 1] + mu;
  if (!(e > floor_)) e = floor_;
  S.e[k - 1] = e;
  for (int i = k - 2; i >= 0; --i) {
    e = (d[i] + mu) - (o[i] * o[i]) / e;
    if (!(e > floor_)) e = floor_;
    S.e[i] = e;
  }
  for (int i = 0; i < k; ++i) S.u[i] = (i & 1) ? -1.0 : 1.0;
  for (int it = 0; it < 4; ++it) {
    double y = S.u[k - 1];
    for (int i = k - 2; i >= 0; --i) { y = S.u[i] - (o[i] / S.e[i + 1]) * y; S.u[i] = y; }
    double x = S.u[0] / S.e[0];
    S.u[0] = x;
    double big = fabs(x);
    for (int i = 1; i < k; ++i) {
      x = S.u[i] / S.e[i] - (o[i - 1] / S.e[i]) * x;
      S.u[i] = x;
      big = fmax(big, fabs(x));
    }
    if (!(big > 0.0) || !(big < HUGE_VAL)) { for (int i = 0; i < k; ++i) S.u[i] = i == 0; big = 1.0; }
    double s = 0.0;
    for (int i = 0; i < k; ++i) { S.u[i] = S.u[i] / big; s += S.u[i] * S.u[i]; }
    const double nrm = sqrt(s);
    for (int i = 0; i < k; ++i) S.u[i] = S.u[i] / nrm;
  }
  double hu = 0.0, hh = 0.0, ug = g0 * S.u[0], uTh = 0.0, uTu = 0.0;
  for (int i = 0; i < k; ++i) {
    const double hi = S.h[i], ui = S.u[i];
    hu += hi * ui;
    hh += hi * hi;
    double th = d[i] * hi, tu = d[i] * ui;
    if (i > 0) { th += o[i - 1] * S.h[i - 1]; tu += o[i - 1] * S.u[i - 1]; }
    if (i + 1 < k) { th += o[i] * S.h[i + 1]; tu += o[i] * S.u[i + 1]; }
    uTh += ui * th;
    uTu += ui * tu;
  }
  const double c = hh - R * R;               // <= 0
  double disc = hu * hu - c;
  if (disc < 0.0) disc = 0.0;
  const double aux = hu + copysign(sqrt(disc), hu);
  double t1 = -aux, t2 = aux != 0.0 ? c / t1 : 0.0;
  const double slope = uTh + ug;
  const double q1 = t1 * slope + 0.5 * (t1 * t1) * uTu;
  const double q2 = t2 * slope + 0.5 * (t2 * t2) * uTu;
  const double tau = q1 <= q2 ? t1 : t2;
  for (int i = 0; i < k; ++i) S.h[i] = S.h[i] + tau * S.u[i];
}

// argmin 1/2 h'T h + g0 h_0 over ||h|| <= R for the k x k tridiagonal in S.d / S.o (filled by
// the caller, visible to every lane).  cols: GLTR_NS columns of k doubles, lane-fastest.  Results
// in S.h and res[0..5] = lambda, ||h||, q_T(h), case, exit path (0 interior, 1 the secular
// iteration converged, 2 near-hard, 3 collapsed bracket), rounds.
__host__ __device__ inline void gltr_tridiag(GltrShared &S, double *cols, int k, double g0,
                                             double R, double *res, int tid) {
  const double *d = S.d, *o = S.o;
  const double R2 = R * R;
  // ---- interior?
  if (GLTR_LANE0) {
    int pd;
    double nn, w3;
    gltr_eval(k, d, o, g0, 0.0, cols, GLTR_NS, 0, pd, nn, w3);
    S.pd0 = pd;
    S.done = pd && sqrt(nn) <= R;
    S.sel = 0;
    S.path = 0;
    S.rounds = 0;
    S.lam[0] = 0.0;
    double tm = 0.0, gl = HUGE_VAL, gu = -HUGE_VAL;
    for (int i = 0; i < k; ++i) {
      const double l = i > 0 ? fabs(o[i - 1]) : 0.0, r = i + 1 < k ? fabs(o[i]) : 0.0;
      tm = fmax(tm, fmax(fabs(d[i]), r));
      gl = fmin(gl, d[i] - (l + r));
      gu = fmax(gu, d[i] + (l + r));
    }
    S.tmax = tm;
    const double pad = 2.0 * GLTR_EPS * k * tm + DBL_MIN;
    S.a = gl - pad;
    S.b = gu + pad;
    S.p = 0.0;
  }
  GLTR_SYNC();
  if (!S.done) {
    // ---- lambda_min(T) in [a, b): count(a) = 0 < count(b)
    if (!S.pd0) {
      const double pivmin = DBL_MIN * fmax(1.0, S.tmax * S.tmax);
      for (int round = 0; round < 12; ++round) {
        const double a = S.a, b = S.b;
        if (!(b - a > GLTR_EPS * S.tmax)) break;
        GLTR_LANES(t, GLTR_NT) {
          const double sigma = a + (b - a) * ((double)(t + 1) / (double)(GLTR_NT + 1));
          S.cnt[t] = gltr_sturm(k, d, o, sigma, pivmin);
        }
        GLTR_SYNC();
        if (GLTR_LANE0) {
          int first = GLTR_NT;
          for (int t = 0; t < GLTR_NT; ++t)
            if (S.cnt[t] > 0) { first = t; break; }
          if (first < GLTR_NT) S.b = a + (b - a) * ((double)(first + 1) / (double)(GLTR_NT + 1));
          if (first > 0) S.a = a + (b - a) * ((double)first / (double)(GLTR_NT + 1));
        }
        GLTR_SYNC();
      }
      if (GLTR_LANE0) S.p = S.a < 0.0 ? -S.a : 0.0;
    }
    if (GLTR_LANE0) {
      const double smin = 4.0 * GLTR_EPS * k * S.tmax + DBL_MIN;
      S.lamL = S.p + smin;
      S.lo = S.p;                       // left of the root: the pole, or 0 with ||h(0)|| > R
      S.hi = g0 / R + S.p;              // ||h(hi)|| <= R
      S.has_newt = 0;
    }
    GLTR_SYNC();
    // ---- the secular equation
    for (int round = 0; round < GLTR_MAX_ROUNDS; ++round) {
      if (GLTR_LANE0) {
        const double smin = S.lamL - S.p;
        S.sa = S.lo - S.p;
        S.sb = S.hi - S.p;
        const double sg = S.sa > smin ? S.sa : smin;
        S.geo = S.sb > 4.0 * sg;
        if (S.geo) {
          double r = S.sb / sg;
          for (int j = 0; j < 6; ++j) r = sqrt(r);      // the 64th root
          S.rt = r;
          S.sa = sg;
        }
        S.lam[0] = S.has_newt ? S.newt : (round == 0 ? S.lamL : S.lo + 0.5 * (S.hi - S.lo));
      }
      GLTR_SYNC();
      GLTR_LANES(t, GLTR_NS) {
        if (t > 0) {
          double s;
          if (S.geo) {
            s = S.sa;
            for (int j = 0; j < t; ++j) s *= S.rt;
          } else {
            s = S.sa + (S.sb - S.sa) * ((double)t / (double)GLTR_NS);
          }
          S.lam[t] = S.p + s;
        }
        int pd;
        double nn, w3;
        gltr_eval(k, d, o, g0, S.lam[t], cols + t, GLTR_NS, 1, pd, nn, w3);
        S.pd[t] = pd;
        S.nn[t] = nn;
        S.w3[t] = w3;
      }
      GLTR_SYNC();
      if (GLTR_LANE0) {
        S.rounds = round + 1;
        int conv = -1, tl = -1, tr = -1;
        double nlo = S.lo, nhi = S.hi;
        for (int t = 0; t < GLTR_NS; ++t) {
          const double lam = S.lam[t];
          if (!(lam > S.lo) || !(lam < S.hi)) continue;      // (outside the bracket: not used)
          const int left = !S.pd[t] || S.nn[t] > R2;
          const double nrm = S.pd[t] ? sqrt(S.nn[t]) : HUGE_VAL;
          if (conv < 0 && S.pd[t] && fabs(nrm - R) <= 1e-12 * R) conv = t;
          if (left) { if (lam > nlo) { nlo = lam; tl = t; } }
          else if (lam < nhi) { nhi = lam; tr = t; }
        }
        const int lamL_right = round == 0 && S.pd[0] && !(S.nn[0] > R2);
        if (conv >= 0) {
          S.done = 1; S.sel = conv; S.path = 1;
        } else if (lamL_right && !S.pd0) {
          S.done = 1; S.sel = 0; S.path = 2;                 // nothing right of the pole
        } else if (!(nlo < nhi) || (tl < 0 && tr < 0)) {
          S.done = 1; S.sel = -1; S.path = 3;                // no shift left between lo and hi
        } else {
          S.has_newt = 0;
          if (tl >= 0 && S.pd[tl] && S.w3[tl] > 0.0) {
            const double nrm = sqrt(S.nn[tl]);
            const double ln = nlo + ((nrm - R) / R) * (S.nn[tl] / S.w3[tl]);
            if (ln > nlo && ln < nhi) { S.newt = ln; S.has_newt = 1; }
          }
          S.lo = nlo;
          S.hi = nhi;
        }
      }
      GLTR_SYNC();
      if (S.done) break;
    }
    if (!S.done) {
      GLTR_SYNC();
      if (GLTR_LANE0) { S.done = 1; S.sel = -1; S.path = 3; }
      GLTR_SYNC();
    }
    if (S.sel < 0) {                     // h(hi) afresh: its column is gone
      if (GLTR_LANE0) {
        int pd;
        double nn, w3;
        gltr_eval(k, d, o, g0, S.hi, cols, GLTR_NS, 0, pd, nn, w3);
        S.lam[0] = S.hi;
        if (!pd)
          for (int i = 0; i < k; ++i) cols[i * GLTR_NS] = 0.0;
      }
      GLTR_SYNC();
    }
  }
  const int sel = S.sel < 0 ? 0 : S.sel;
  GLTR_LANES(i, k) S.h[i] = cols[i * GLTR_NS + sel];
  GLTR_SYNC();
  if (GLTR_LANE0) {
    if (S.path >= 2) gltr_eig_step(S, k, g0, R, S.lamL);
    double hh = 0.0, q = 0.0;
    for (int i = 0; i < k; ++i) {
      const double hi = S.h[i];
      hh += hi * hi;
      double th = d[i] * hi;
      if (i + 1 < k) th += 2.0 * (o[i] * S.h[i + 1]);
      q += hi * th;
    }
    res[0] = S.lam[sel];
    res[1] = sqrt(hh);
    res[2] = 0.5 * q + g0 * S.h[0];
    res[3] = S.path == 0 ? 0.0 : S.path == 1 ? 1.0 : 2.0;
    res[4] = (double)S.path;
    res[5] = (double)S.rounds;
  }
  GLTR_SYNC();
}

int gltr_grid(int64_t n) { return ipx_grid_for(n, IPX_BLOCK * 4, IPX_VEC_GRID_CAP); }

size_t gltr_lds_bytes(int k) { return (size_t)GLTR_NS * (size_t)k * sizeof(double); }

template <auto KERNEL>
void gltr_allow_lds() {
  static bool set = false;
  if (set) return;
  (void)hipFuncSetAttribute((const void *)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)gltr_lds_bytes(GLTR_MAXV));
  set = true;
}

// ---- start: gamma_0, q_0, the header ------------------------------------------------------
__global__ void __launch_bounds__(IPX_BLOCK)
k_gltr_sumsq(int64_t n, const double *__restrict__ g, double *__restrict__ part) {
  __shared__ double red[IPX_BLOCK / IPX_WAVE];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * IPX_BLOCK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * IPX_BLOCK) {
    const double v = g[i];
    acc += v * v;
  }
  acc = ipx_block_reduce<IPX_SUM>(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

__global__ void __launch_bounds__(IPX_BLOCK)
k_gltr_start(int64_t n, int kmax, int cap, const double *__restrict__ g, double *__restrict__ Q,
             double *__restrict__ state, const double *__restrict__ part, double radius,
             double tol) {
  __shared__ double red[IPX_BLOCK / IPX_WAVE];
  const double gg = ipx_sum_partials<IPX_SUM>(part, gridDim.x, red);
  const double g0 = sqrt(gg);
  for (int64_t i = (int64_t)blockIdx.x * IPX_BLOCK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * IPX_BLOCK)
    Q[i] = g0 > 0.0 ? g[i] / g0 : 0.0;
  if (blockIdx.x == 0) {
    const double t = tol >= 0.0 ? tol : fmax(fmin(0.01 * g0, 0.1 * gg), 1e-25);
    for (int j = threadIdx.x; j < GLTR_HDR + 3 * kmax; j += IPX_BLOCK) {
      double v = 0.0;
      if (j == 0) v = (gg < t || cap < 1) ? (gg < t ? 4.0 : 1.0) : 0.0;
      else if (j == 2) v = g0;
      else if (j == 3) v = radius;
      else if (j == 4) v = t;
      else if (j == 10) v = (double)cap;
      state[j] = v;
    }
  }
}

// ---- one step --------------------------------------------------------------------------------
__global__ void __launch_bounds__(IPX_BLOCK)
k_gltr_delta(int64_t n, int kmax, const double *__restrict__ w, const double *__restrict__ Q,
             const double *__restrict__ state, double *__restrict__ part) {
  if (state[0] != 0.0) return;
  const int k = (int)state[1];
  if (k >= kmax) return;
  __shared__ double red[IPX_BLOCK / IPX_WAVE];
  const double *q = Q + (int64_t)k * n;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * IPX_BLOCK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * IPX_BLOCK)
    acc += q[i] * w[i];
  acc = ipx_block_reduce<IPX_SUM>(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

__global__ void __launch_bounds__(IPX_BLOCK)
k_gltr_update(int64_t n, int kmax, const double *__restrict__ w, double *__restrict__ Q,
              const double *__restrict__ state, double *__restrict__ part) {
  if (state[0] != 0.0) return;
  const int k = (int)state[1];
  if (k >= kmax) return;
  __shared__ double red[IPX_BLOCK / IPX_WAVE];
  const int G = gridDim.x;
  const double delta = ipx_sum_partials<IPX_SUM>(part, G, red);
  const double gk = k > 0 ? state[GLTR_HDR + kmax + (k - 1)] : 0.0;
  const double *q = Q + (int64_t)k * n;
  const double *qm = Q + (int64_t)(k > 0 ? k - 1 : 0) * n;
  double *out = Q + (int64_t)(k + 1) * n;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * IPX_BLOCK + threadIdx.x; i < n;
       i += (int64_t)G * IPX_BLOCK) {
    double v = w[i] - delta * q[i];
    if (k > 0) v = v - gk * qm[i];
    out[i] = v;
    acc += v * v;
  }
  acc = ipx_block_reduce<IPX_SUM>(acc, red);
  if (threadIdx.x == 0) part[G + blockIdx.x] = acc;
}

__global__ void __launch_bounds__(IPX_BLOCK)
k_gltr_solve(int kmax, int G, double *__restrict__ state, const double *__restrict__ part) {
  if (state[0] != 0.0) return;
  const int k = (int)state[1];
  if (k >= kmax) return;
  extern __shared__ __attribute__((aligned(16))) double gltr_cols[];
  __shared__ GltrShared S;
  __shared__ double red[IPX_BLOCK / IPX_WAVE];
  __shared__ double res[8];
  const int tid = threadIdx.x;
  const double delta = ipx_sum_partials<IPX_SUM>(part, G, red);
  const double ww = ipx_sum_partials<IPX_SUM>(part + G, G, red);
  const double gnext = sqrt(ww);
  double *diag = state + GLTR_HDR, *off = diag + kmax, *h = off + kmax;
  const int kk = k + 1;
  for (int i = tid; i < kk; i += IPX_BLOCK) {
    S.d[i] = i == k ? delta : diag[i];
    S.o[i] = i == k ? gnext : off[i];
  }
  __syncthreads();
  const double g0 = state[2], R = state[3], tol = state[4];
  gltr_tridiag(S, gltr_cols, kk, g0, R, res, tid);
  for (int i = tid; i < kk; i += IPX_BLOCK) h[i] = S.h[i];
  if (tid == 0) {
    diag[k] = delta;
    off[k] = gnext;
    const double crit = gnext * S.h[k];
    const int cap = (int)state[10];
    double stop = 0.0;
    if (gnext <= 1e-14 * g0 || crit * crit < tol) stop = 4.0;
    else if (kk >= cap || kk >= kmax) stop = 1.0;
    state[1] = (double)kk;
    state[5] = res[0];
    state[6] = res[1];
    state[7] = res[2];
    state[8] = gnext;
    state[9] = res[3];
    state[11] = res[4];
    state[12] = res[5];
    state[13] = delta;
    state[0] = stop;
  }
}

__global__ void __launch_bounds__(IPX_BLOCK)
k_gltr_next(int64_t n, int kmax, double *__restrict__ Q, const double *__restrict__ state) {
  if (state[0] != 0.0) return;
  const int k = (int)state[1];
  if (k > kmax || k < 1) return;
  const double g = state[8];
  double *q = Q + (int64_t)k * n;
  for (int64_t i = (int64_t)blockIdx.x * IPX_BLOCK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * IPX_BLOCK)
    q[i] = q[i] / g;
}

// ---- x = x0 + Q h --------------------------------------------------------------------------
// V = 2: two elements per lane in 16-byte accesses (n even, every base 16-byte aligned)
template <int V>
__global__ void __launch_bounds__(IPX_BLOCK)
k_gltr_combine(int64_t n, int kmax, const double *__restrict__ Q,
               const double *__restrict__ state, const double *__restrict__ x0,
               double *__restrict__ x) {
  __shared__ double hs[GLTR_MAXV];
  int k = (int)state[1];
  if (k > kmax) k = kmax;
  const double *h = state + GLTR_HDR + 2 * (int64_t)kmax;
  for (int j = threadIdx.x; j < k; j += IPX_BLOCK) hs[j] = h[j];
  __syncthreads();
  const int64_t nv = n / V;
  for (int64_t i = (int64_t)blockIdx.x * IPX_BLOCK + threadIdx.x; i < nv;
       i += (int64_t)gridDim.x * IPX_BLOCK) {
    if (V == 2) {
      double2 acc = x0 ? ((const double2 *)x0)[i] : make_double2(0.0, 0.0);
      const double2 *col = (const double2 *)Q + i;
      int j = 0;
      for (; j + 4 <= k; j += 4) {           // four columns in flight, added left to right
        const double2 c0 = col[(int64_t)j * nv], c1 = col[(int64_t)(j + 1) * nv];
        const double2 c2 = col[(int64_t)(j + 2) * nv], c3 = col[(int64_t)(j + 3) * nv];
        acc.x = acc.x + hs[j] * c0.x;         acc.y = acc.y + hs[j] * c0.y;
        acc.x = acc.x + hs[j + 1] * c1.x;     acc.y = acc.y + hs[j + 1] * c1.y;
        acc.x = acc.x + hs[j + 2] * c2.x;     acc.y = acc.y + hs[j + 2] * c2.y;
        acc.x = acc.x + hs[j + 3] * c3.x;     acc.y = acc.y + hs[j + 3] * c3.y;
      }
      for (; j < k; ++j) {
        const double2 c = col[(int64_t)j * nv];
        acc.x = acc.x + hs[j] * c.x;
        acc.y = acc.y + hs[j] * c.y;
      }
      ((double2 *)x)[i] = acc;
    } else {
      double acc = x0 ? x0[i] : 0.0;
      int j = 0;
      for (; j + 4 <= k; j += 4) {
        const double c0 = Q[(int64_t)j * n + i], c1 = Q[(int64_t)(j + 1) * n + i];
        const double c2 = Q[(int64_t)(j + 2) * n + i], c3 = Q[(int64_t)(j + 3) * n + i];
        acc = acc + hs[j] * c0;
        acc = acc + hs[j + 1] * c1;
        acc = acc + hs[j + 2] * c2;
        acc = acc + hs[j + 3] * c3;
      }
      for (; j < k; ++j) acc = acc + hs[j] * Q[(int64_t)j * n + i];
      x[i] = acc;
    }
  }
}

// ---- the tridiagonal solve alone ------------------------------------------------------------
__global__ void __launch_bounds__(IPX_BLOCK)
k_gltr_tridiag(int k, const double *__restrict__ diag, const double *__restrict__ off, double g0,
               double R, double *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) double gltr_cols[];
  __shared__ GltrShared S;
  __shared__ double res[8];
  const int tid = threadIdx.x;
  for (int i = tid; i < k; i += IPX_BLOCK) {
    S.d[i] = diag[i];
    S.o[i] = i + 1 < k ? off[i] : 0.0;
  }
  __syncthreads();
  gltr_tridiag(S, gltr_cols, k, g0, R, res, tid);
  for (int i = tid; i < k; i += IPX_BLOCK) out[8 + i] = S.h[i];
  if (tid < 8) out[tid] = tid < 6 ? res[tid] : 0.0;
}

bool gltr_args_ok(int64_t n, int kmax) { return n > 0 && kmax >= 1 && kmax <= GLTR_MAXV; }

}  // namespace

extern "C" {

int64_t ipx_gltr_state_doubles(int32_t kmax) { return GLTR_HDR + 3 * (int64_t)kmax; }

int ipx_gltr_grid(int64_t n) { return gltr_grid(n); }

int64_t ipx_gltr_part_doubles(int64_t n) { return 2 * (int64_t)gltr_grid(n); }

int ipx_gltr_start(int64_t n, int32_t kmax, int32_t cap, const double *g, double *Q, double *state,
                   double *part, double radius, double tol, void *stream) {
  if (!gltr_args_ok(n, kmax) || !g || !Q || !state || !part || !(radius >= 0.0)) return IPX_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(gltr_grid(n)), block(IPX_BLOCK);
  hipLaunchKernelGGL(k_gltr_sumsq, grid, block, 0, st, n, g, part);
  IPX_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_gltr_start, grid, block, 0, st, n, (int)kmax, (int)cap, g, Q, state,
                     (const double *)part, radius, tol);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

int ipx_gltr_step(int64_t n, int32_t kmax, const double *w, double *Q, double *state, double *part,
                  void *stream) {
  if (!gltr_args_ok(n, kmax) || !w || !Q || !state || !part) return IPX_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int G = gltr_grid(n);
  const dim3 grid(G), block(IPX_BLOCK);
  gltr_allow_lds<k_gltr_solve>();
  hipLaunchKernelGGL(k_gltr_delta, grid, block, 0, st, n, (int)kmax, w, (const double *)Q,
                     (const double *)state, part);
  IPX_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_gltr_update, grid, block, 0, st, n, (int)kmax, w, Q, (const double *)state,
                     part);
  IPX_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_gltr_solve, dim3(1), block, gltr_lds_bytes(kmax), st, (int)kmax, G, state,
                     (const double *)part);
  IPX_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_gltr_next, grid, block, 0, st, n, (int)kmax, Q, (const double *)state);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

int ipx_gltr_combine(int64_t n, int32_t kmax, const double *Q, const double *state,
                     const double *x0, double *x, void *stream) {
  if (!gltr_args_ok(n, kmax) || !Q || !state || !x) return IPX_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const bool wide = n % 2 == 0 && ((uintptr_t)Q % 16 == 0) && ((uintptr_t)x % 16 == 0) &&
                    ((uintptr_t)x0 % 16 == 0);
  const dim3 block(IPX_BLOCK);
  if (wide) {
    hipLaunchKernelGGL(k_gltr_combine<2>, dim3(ipx_grid_for(n / 2, IPX_BLOCK, 1 << 20)), block, 0,
                       st, n, (int)kmax, Q, state, x0, x);
  } else {
    hipLaunchKernelGGL(k_gltr_combine<1>, dim3(ipx_grid_for(n, IPX_BLOCK, 1 << 20)), block, 0, st,
                       n, (int)kmax, Q, state, x0, x);
  }
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

int ipx_gltr_tridiag(int32_t k, const double *diag, const double *off, double g0, double radius,
                     double *out, void *stream) {
  if (k < 1 || k > GLTR_MAXV || !diag || (k > 1 && !off) || !out || !(g0 > 0.0) || !(radius > 0.0))
    return IPX_EINVAL;
  gltr_allow_lds<k_gltr_tridiag>();
  hipLaunchKernelGGL(k_gltr_tridiag, dim3(1), dim3(IPX_BLOCK), gltr_lds_bytes(k),
                     (hipStream_t)stream, (int)k, diag, off, g0, radius, out);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

int ipx_gltr_tridiag_host(int32_t k, const double *diag, const double *off, double g0,
                          double radius, double *out) {
  if (k < 1 || k > GLTR_MAXV || !diag || (k > 1 && !off) || !out || !(g0 > 0.0) || !(radius > 0.0))
    return IPX_EINVAL;
  std::vector<double> cols((size_t)GLTR_NS * k);
  std::vector<GltrShared> Sv(1);
  GltrShared &S = Sv[0];
  for (int i = 0; i < k; ++i) {
    S.d[i] = diag[i];
    S.o[i] = i + 1 < k ? off[i] : 0.0;
  }
  double res[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  gltr_tridiag(S, cols.data(), k, g0, radius, res, 0);
  for (int i = 0; i < 8; ++i) out[i] = res[i];
  for (int i = 0; i < k; ++i) out[8 + i] = S.h[i];
  return IPX_OK;
}

}  // extern "C"
