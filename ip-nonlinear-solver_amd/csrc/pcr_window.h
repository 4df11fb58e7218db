// The pieces of the parallel cyclic reduction (PCR) on one window of a tridiagonal S = A A', each
// written ONCE: the kernels of banded.hip that work on such windows -- k_pcr_check (the factor-
// time level search), k_solve_pcr (the solve with its tails) and k_step1_solve_tail (the
// projection half of a CG iteration) -- must agree bit for bit, so every rounding they share is
// formed here.  (k_step1_solve_tail, the hot one, calls pcr_levels and keeps the other pieces
// written out, in step with these: see the note at its head.)  Device helpers only: the kernels
// keep their own LDS arrays, barriers between phases, early returns and the order of their first
// loads.
// csrc/resident.hip carries a reduction of its own on purpose (its loads are batched ahead of the
// arithmetic, its padding is H rows, not PCR_PAD, and it hides indices from the compiler): sharing
// more than the reciprocal (ipx_rcp_newton, ipx_common.h) would make these helpers branch on
// their caller.
#pragma once
#include "ipx_common.h"

typedef double v2d __attribute__((ext_vector_type(2)));

constexpr int PCR_LMAX = 7;                 // reduction distance up to 2^7 = 128 rows
constexpr int PCR_PAD = 1 << PCR_LMAX;      // identity rows either side of a window in LDS

// Window `wg` of a reduction to level L of a matrix of m rows, as lane `lane` of its workgroup
// sees it: the workgroup's own rows [wg rows_wg, (wg + 1) rows_wg), as far as the matrix has
// them, and H = 2^L halo rows either side, R rows in all.  A lane works on window rows lane +
// k TB; the global row of a window row is formed from the LANE's row, a vector register (formed
// from the window's first row, a scalar, the compiler carries differences like m - g0 in scalar
// registers through a whole kernel).
struct PcrWindow {
  int H, R, rows_wg, m, lane;
  int64_t lane_row;                                  // global row of window row `lane`
  __device__ __forceinline__ PcrWindow(int wg, int rows_wg_, int L, int m_, int lane_)
      : H(1 << L), R(rows_wg_ + 2 * (1 << L)), rows_wg(rows_wg_), m(m_), lane(lane_),
        lane_row((int64_t)wg * rows_wg_ - (1 << L) + lane_) {}
  // global row of window row r (negative or >= m outside the matrix)
  __device__ __forceinline__ int64_t row(int r) const { return lane_row + (r - lane); }
  __device__ __forceinline__ bool inside(int r) const {
    const int64_t g = row(r);
    return r < R && g >= 0 && g < m;
  }
  // the row every load of window row r goes to: clamped into the matrix, no bounds branches
  __device__ __forceinline__ int64_t clamped(int r) const {
    return min(max(row(r), (int64_t)0), (int64_t)m - 1);
  }
  __device__ __forceinline__ bool own(int r) const {
    return r >= H && r < H + rows_wg && row(r) < m;
  }
  // sub-diagonal a = S[g][g - 1] and diagonal b of window row r.  Rows outside the window or the
  // matrix are identity rows (a = 0, b = 1); the coupling of row 0 of the window to the row
  // before it is cut, and so is that of the matrix's first row.  Returns whether the row exists.
  __device__ __forceinline__ bool row_load(const double *__restrict__ band, int r, double &a,
                                           double &b) const {
    const int64_t g = row(r);
    const bool in = inside(r);
    const int64_t gc = clamped(r);
    const double bv = band[gc], av = band[(int64_t)m + gc];
    a = (in && g >= 1 && r >= 1) ? av : 0.0;
    b = in ? bv : 1.0;
    return in;
  }
};

// identity padding of the ping-pong buffers: rows [-PCR_PAD, 0) and [R, R + PCR_PAD) of both
// (a = 0, 1 / b = 1, d = 0); storage index = window row + PCR_PAD
template <int TB, bool WITH_D, int RS>
__device__ __forceinline__ void pcr_pad_identity(int R, int tid, double (&pa)[2][RS],
                                                 double (&pr)[2][RS],
                                                 double (*pd)[RS] = nullptr) {
  for (int i = tid; i < 2 * PCR_PAD; i += TB) {
    const int r = i < PCR_PAD ? i : R + i;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      pa[u][r] = 0.0; pr[u][r] = 1.0;
      if constexpr (WITH_D) pd[u][r] = 0.0;
    }
  }
}

// One elimination step of a row against its neighbours at distance h -- the reduction's roundings.
// The matrix is symmetric: only the sub-diagonal a_i = S[i][i-h] is carried (the coupling upwards
// is a_{i+h}, read from the neighbour), with the reciprocal r = 1 / b of the diagonal next to it:
//     al = -a_i r_{i-h},  ga = -a_{i+h} r_{i+h}
//     b_i <- b_i + al a_i + ga a_{i+h},  d_i <- d_i + al d_{i-h} + ga d_{i+h},  a_i <- al a_{i-h}
// WITH_D = false: the matrix alone (k_pcr_check), d / dlo / dhi are not touched.
template <bool WITH_D>
__device__ __forceinline__ void pcr_eliminate(double &a, double &b, double &d, double alo,
                                              double rlo, double dlo, double ahi, double rhi,
                                              double dhi) {
  const double al = -a * rlo, ga = -ahi * rhi;
  double bn = __builtin_fma(al, a, b);
  bn = __builtin_fma(ga, ahi, bn);
  if constexpr (WITH_D) {
    double dn = __builtin_fma(al, dlo, d);
    dn = __builtin_fma(ga, dhi, dn);
    d = dn;
  }
  a = al * alo;
  b = bn;
}

// The L reduction levels of a solve on one window: lane t carries window rows t + k TB in
// a / b / d; the two LDS buffers alternate by level (one LDS barrier per level), their identity
// padding is the caller's (pcr_pad_identity).
template <int NR, int TB, int RS>
__device__ __forceinline__ void pcr_levels(int L, int R, int tid, double (&a)[NR], double (&b)[NR],
                                           double (&d)[NR], double (&pa)[2][RS],
                                           double (&pr)[2][RS], double (&pd)[2][RS]) {
  for (int s = 0; s < L; ++s) {
    const int h = 1 << s, cur = s & 1;
    double rc[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      const int r = tid + k * TB;
      rc[k] = ipx_rcp_newton(b[k]);
      if (r < R) {
        pa[cur][PCR_PAD + r] = a[k]; pr[cur][PCR_PAD + r] = rc[k]; pd[cur][PCR_PAD + r] = d[k];
      }
    }
    ipx_lds_barrier();
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      const int r = PCR_PAD + min(tid + k * TB, R - 1);
      const double alo = pa[cur][r - h], rlo = pr[cur][r - h], dlo = pd[cur][r - h];
      const double ahi = pa[cur][r + h], rhi = pr[cur][r + h], dhi = pd[cur][r + h];
      pcr_eliminate<true>(a[k], b[k], d[k], alo, rlo, dlo, ahi, rhi, dhi);
    }
  }
}

// x = d / b after the last level: the whole window to LDS (sx, for the tails and the residual),
// the own rows to memory
template <int NR, int TB>
__device__ __forceinline__ void pcr_solution_to_lds(const PcrWindow &win, int tid,
                                                    const double (&d)[NR], const double (&b)[NR],
                                                    double *sx, double *__restrict__ x) {
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    const int r = tid + k * TB;
    if (r < win.R) {
      const double xv = d[k] / b[k];
      sx[r] = xv;
      if (win.own(r)) x[win.row(r)] = xv;
    }
  }
}

// The workgroup's sum of v to part[wg], with a zero in the second plane (the compensation slot
// of the reductions that read these partials)
template <int TB>
__device__ __forceinline__ void pcr_partial_pair(double v, double *red_lds, double *part, int wg,
                                                 int nwin, int tid) {
  const double tot = ipx_block_reduce<IPX_SUM>(v, red_lds);
  if (tid == 0) {
    part[wg] = tot;
    part[nwin + wg] = 0.0;
  }
}

// g = sign (r - A'v) on the variables [av0, av0 + avn) a workgroup owns, v out of LDS.  A lane
// takes PAIRS of consecutive variables, QP of them (16-byte loads of the values and of whatever
// else the kernel reads per variable, 4-byte loads of the two 16-bit row offsets: half the load
// instructions -- the tail is bound by the CU's load issue); pairs start at an even variable so
// that every load is naturally aligned (the planes are padded to even length), possibly one
// before av0.  A' in ELL(2) form: variable j has its first constraint at window row H +
// ell_row[j] and the row after it, values ell_val[j] and ell_val[ell_n + j]; an absent entry
// carries value 0: same sum as the CSR row.
template <int QP, int TB>
struct PcrPairTail {
  int av0, avn;
  int64_t vb;                                        // the first pair
  unsigned ac[QP];                                   // (two 16-bit row offsets)
  v2d aw0[QP], aw1[QP];
  // The loads, to be issued early enough to arrive while the reduction runs; more(k, j) issues
  // the caller's own loads for pair k at variable j (clamped to the workgroup's last pair) after
  // them.
  template <class More>
  __device__ __forceinline__ void load(const uint16_t *__restrict__ ell_row,
                                       const double *__restrict__ ell_val, int64_t ell_n,
                                       int av0_, int avn_, int tid, More more) {
    av0 = av0_; avn = avn_;
    vb = av0 & ~1;
    const int64_t last = max((int64_t)av0 + avn - 1, vb) & ~(int64_t)1;
#pragma unroll
    for (int k = 0; k < QP; ++k) {
      const int64_t j = min(vb + 2 * (int64_t)(tid + k * TB), last);
      ac[k] = *reinterpret_cast<const unsigned *>(ell_row + j);
      aw0[k] = *reinterpret_cast<const v2d *>(ell_val + j);
      aw1[k] = *reinterpret_cast<const v2d *>(ell_val + ell_n + j);
      more(k, j);
    }
  }
  // The lane's pairs: y = -sign (A'v) + sign r with r = r_of(k, j, half) for variable j + half,
  // stored to g_out where the variable is the workgroup's (a pair that reaches into a
  // neighbour's variables reads that workgroup's offsets -- in range, result unused); returns
  // the lane's sum of y^2 in the order of the variables.  extra(k, in0, in1) is called per pair
  // with what is owned.
  template <class ROf, class Extra>
  __device__ __forceinline__ double apply(const double *sx, int H, double sign, int tid,
                                          double *__restrict__ g_out, ROf r_of,
                                          Extra extra) const {
    double gacc = 0.0;
#pragma unroll
    for (int k = 0; k < QP; ++k) {
      const int64_t j = vb + 2 * (int64_t)(tid + k * TB);
      const int c0 = H + (int)(ac[k] & 0xffffu), c1 = H + (int)(ac[k] >> 16);
      double y0 = -sign * (aw0[k].x * sx[c0] + aw1[k].x * sx[c0 + 1]);
      y0 += sign * r_of(k, j, 0);
      double y1 = -sign * (aw0[k].y * sx[c1] + aw1[k].y * sx[c1 + 1]);
      y1 += sign * r_of(k, j, 1);
      const bool in0 = j >= av0 && j < (int64_t)av0 + avn;
      const bool in1 = j + 1 >= av0 && j + 1 < (int64_t)av0 + avn;
      if (in0 && in1) {
        *reinterpret_cast<v2d *>(g_out + j) = (v2d){y0, y1};
        gacc += y0 * y0;
        gacc += y1 * y1;
      } else if (in0) {
        g_out[j] = y0;
        gacc += y0 * y0;
      } else if (in1) {
        g_out[j + 1] = y1;
        gacc += y1 * y1;
      }
      extra(k, in0, in1);
    }
    return gacc;
  }
};

// The lane's part of ||w - S x||^2 over the own rows:  w_i - (a_i x_{i-1} + b_i x_i + a_{i+1}
// x_{i+1}) from the level-0 rows a0 / b0 / w0 kept in registers and x in LDS (sx); a_{i+1} is
// the neighbouring lane's, handed over through pa0 (a buffer of the reduction, free by now;
// its padding is still a = 0).  One LDS barrier.
template <int NR, int TB>
__device__ __forceinline__ double pcr_own_residual(const PcrWindow &win, int tid,
                                                   const double (&a0)[NR], const double (&b0)[NR],
                                                   const double (&w0)[NR], double *pa0,
                                                   const double *sx) {
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    const int r = tid + k * TB;
    if (r < win.R) pa0[PCR_PAD + r] = a0[k];
  }
  ipx_lds_barrier();
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    const int r = tid + k * TB;
    if (win.own(r)) {
      double sum = b0[k] * sx[r];
      sum += a0[k] * sx[r - 1];
      sum += pa0[PCR_PAD + r + 1] * sx[r + 1];
      const double res = w0[k] - sum;
      acc += res * res;
    }
  }
  return acc;
}
