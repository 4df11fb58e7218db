// Linked direct (A A')^-1: a few dense rows on top of a banded / block-tridiagonal solve.
//
// The rows of A are band rows B (m_B of them) and q <= 32 link rows D, in any positions:
//     S = A A' = [ S_B  E ]     S_B = B B' (what the direct solvers factor),
//                [ E'   F ]     E = B D' (m_B x q),  F = D D' (q x q),
//     Y = S_B^-1 E,  K = F - E' Y,   u = S_B^-1 w_B,  t = w_D - Y' w_B,  K z = t,
//     v_B = u - Y z,  v_D = z
// -- a block Cholesky of an SPD matrix (K is the Schur complement: SPD, K <= F).  The inner
// solves are the caller's; Python owns every buffer, nothing is allocated, no handle is kept.
//
// Storage.  D' is a dense n x q array, ROW-major (D'[c, j] at c * q + j): the q lanes of a row
// group gather one contiguous run of q doubles per entry of A.  G = P A D' is column-major with
// leading dimension m = m_B + q, P the row map `dst_row` (band rows to 0 .. m_B - 1 in their
// order, link rows to m_B .. m - 1): the first m_B entries of a column are a column of E, the
// last q a column of F.  Y has the same shape with q ZERO rows at the end, and the gathered w_B
// has q zeros at the end, so that ipx_border_gram(m, q, G, Y) and ipx_border_tdot(m, q, Y, w_B)
// (csrc/bordered.hip: one m for the row count and the leading dimension) read them in place:
// the last q rows add F[., a] * 0 and 0 * 0 to a sum, which does not change it.
//
//   ipx_link_spmm    G = P A D': a group of 32 lanes per row, lane j the column j of D'.  The
//                    lanes load 32 entries (value, column) of the row at once and hand them
//                    round by a shuffle: A is read once for all q.  Entry (r, j) is the sum over
//                    the row's entries in storage order, one multiply and one add each.
//   ipx_link_chol    K = F - sum_g part[g] (ascending g; part: ipx_border_gram's blocks), its
//                    Cholesky factor in LDS, pivot bits and max_j F_jj / K_jj.  One workgroup.
//   ipx_link_apply   every workgroup folds the partials of Y' w_B in the order of
//                    ipx_border_apply, forms t, solves L L' z = t in wave 0 and writes
//                    v[b_rows[r]] = u[r] - sum_j Y[r, j] z[j] (j ascending); group 0 writes
//                    v[d_rows[j]] = z[j].
//
// Every sum has a fixed order, there are no atomics, divisions and square roots are correctly
// rounded: the same values give the same bits, and A scaled by 2^s gives Y unchanged, K and L
// scaled by 4^s and 2^s, bit for bit.  Pivot signals of K: bit 0 -- a pivot below 2^-43 of F_jj
// (the diagonal entry of S); bits 0 and 2 -- a pivot <= 0 (1 takes its place: nothing faults).
#include "ipx_common.h"

namespace {

constexpr int LK_QMAX = 32;                    // ipx_border_pmax()
constexpr int LK_LANES = 32;                   // lanes of a row group in the product
constexpr int LK_ROWS = IPX_BLOCK / LK_LANES;  // rows of a workgroup in the product
constexpr int LK_CHUNK = IPX_BLOCK;            // ipx_border_rows_per_group(): a row per lane
constexpr int LK_APPLY_CAP = 1024;             // workgroups of the apply kernel, at most
constexpr int LK_PAD = LK_QMAX + 1;            // LDS row stride (doubles)
constexpr int LK_FOLD = IPX_BLOCK / LK_QMAX;   // 8 strided partial sums per entry of t

// G[dst_row[r] + m j] = sum_e val[e] * Dt[colidx[e] q + j], e over row r in storage order
__global__ void __launch_bounds__(IPX_BLOCK)
k_lk_spmm(int64_t m, int q, const int32_t *__restrict__ rowptr,
          const int32_t *__restrict__ colidx, const double *__restrict__ val,
          const double *__restrict__ Dt, const int32_t *__restrict__ dst_row,
          double *__restrict__ G) {
  const int j = threadIdx.x & (LK_LANES - 1);
  const int64_t r = (int64_t)blockIdx.x * LK_ROWS + (threadIdx.x / LK_LANES);
  if (r >= m) return;                                   // (uniform in the row group)
  const double *__restrict__ Dj = Dt + (j < q ? j : q - 1);   // idle lanes read a valid column
  const int e1 = rowptr[r + 1];
  double acc = 0.0;
  for (int e = rowptr[r]; e < e1; e += LK_LANES) {
    const int cnt = e1 - e < LK_LANES ? e1 - e : LK_LANES;    // (uniform in the row group)
    int c = 0;
    double a = 0.0;
    if (j < cnt) {
      c = colidx[e + j];
      a = val[e + j];
    }
    if (cnt == LK_LANES) {
#pragma unroll 8
      for (int t = 0; t < LK_LANES; ++t) {
        const double d = Dj[(int64_t)__shfl(c, t, LK_LANES) * q];
        acc = acc + __shfl(a, t, LK_LANES) * d;
      }
    } else {
      for (int t = 0; t < cnt; ++t) {
        const double d = Dj[(int64_t)__shfl(c, t, LK_LANES) * q];
        acc = acc + __shfl(a, t, LK_LANES) * d;
      }
    }
  }
  if (j < q) G[(int64_t)dst_row[r] + m * j] = acc;
}

// K = F - sum_g part[g] (ascending g; F = the last q rows of G), L = chol(K) (lower, row-major;
// zeros above the diagonal), info[0] = pivot bits, info[1] = max_j F_jj / K_jj.  One workgroup.
__global__ void __launch_bounds__(IPX_BLOCK)
k_lk_chol(int64_t m, int q, int groups, const double *__restrict__ G,
          const double *__restrict__ part, double *__restrict__ K, double *__restrict__ L,
          double *__restrict__ info) {
  __shared__ double T[LK_QMAX * LK_PAD], colv[LK_QMAX], f0[LK_QMAX], k0[LK_QMAX];
  const int tid = threadIdx.x, qq = q * q;
  for (int e = tid; e < qq; e += IPX_BLOCK) {
    double s = 0.0;
#pragma unroll 8
    for (int g = 0; g < groups; ++g) s += part[(int64_t)g * qq + e];
    const int a = e / q, b = e % q;
    const double f = G[(m - q + a) + m * b];
    const double k = f - s;
    K[e] = k;
    T[a * LK_PAD + b] = k;
    if (a == b) {
      f0[a] = f;
      k0[a] = k;
    }
  }
  __syncthreads();
  int bits = 0;
  if (tid == 0) {
    double worst = 0.0;
    for (int j = 0; j < q; ++j) {
      const double c = k0[j] > 0.0 ? f0[j] / k0[j] : __builtin_huge_val();
      worst = c > worst ? c : worst;
    }
    info[1] = worst;
  }
  // right-looking Cholesky on the lower triangle, a column per trip (as csrc/bordered.hip)
  for (int j = 0; j < q; ++j) {
    const double d = T[j * LK_PAD + j];
    if (tid == 0 && !(d > IPX_PIVOT_RTOL * f0[j])) bits |= (d > 0.0) ? 1 : 5;
    const double l = sqrt(d > 0.0 ? d : 1.0);
    if (tid >= j && tid < q) colv[tid] = tid == j ? l : T[tid * LK_PAD + j] / l;
    __syncthreads();
    const int rem = q - j - 1;
    for (int e = tid; e < rem * rem; e += IPX_BLOCK) {
      const int i = j + 1 + e / rem, c = j + 1 + e % rem;
      if (c <= i) T[i * LK_PAD + c] = __builtin_fma(-colv[i], colv[c], T[i * LK_PAD + c]);
    }
    if (tid >= j && tid < q) T[tid * LK_PAD + j] = colv[tid];
    __syncthreads();
  }
  for (int e = tid; e < qq; e += IPX_BLOCK) {
    const int r = e / q, c = e % q;
    L[e] = c <= r ? T[r * LK_PAD + c] : 0.0;
  }
  if (tid == 0) info[0] = (double)bits;
}

// t = w_D - (the partials folded), z = (L L')^-1 t, v[b_rows[r]] = u[r] - sum_j Y[r, j] z[j]
// (j ascending), v[d_rows[j]] = z[j] (workgroup 0)
__global__ void __launch_bounds__(IPX_BLOCK)
k_lk_apply(int64_t m, int q, int groups, const double *__restrict__ Y,
           const double *__restrict__ L, const double *__restrict__ part,
           const double *__restrict__ u, const double *__restrict__ w,
           const int32_t *__restrict__ b_rows, const int32_t *__restrict__ d_rows,
           double *__restrict__ v) {
  __shared__ double Ls[LK_QMAX * LK_PAD], fold[LK_FOLD * LK_QMAX], z[LK_QMAX];
  const int tid = threadIdx.x;
  const int64_t mB = m - q;
  for (int e = tid; e < q * q; e += IPX_BLOCK) Ls[(e / q) * LK_PAD + e % q] = L[e];
  {
    // entry j of Y' w_B: 8 lanes take the groups g = s, s + 8, ... in ascending order, then the
    // 8 sums are added in ascending s -- the order of ipx_border_apply, the same in every group
    const int j = tid % LK_QMAX, s8 = tid / LK_QMAX;
    double s = 0.0;
    if (j < q)
      for (int g = s8; g < groups; g += LK_FOLD) s += part[(int64_t)g * q + j];
    fold[s8 * LK_QMAX + j] = s;
  }
  __syncthreads();
  if (tid < IPX_WAVE) {                                       // wave 0, every lane active
    const int lane = tid;
    double ti = 0.0;
    if (lane < q) {
      double s = fold[lane];
      for (int s8 = 1; s8 < LK_FOLD; ++s8) s += fold[s8 * LK_QMAX + lane];
      ti = w[d_rows[lane]] - s;
    }
    for (int k = 0; k < q; ++k) {                             // L y = t
      const double yk = __shfl(ti, k) / Ls[k * LK_PAD + k];
      if (lane == k) ti = yk;
      else if (lane > k && lane < q) ti = __builtin_fma(-Ls[lane * LK_PAD + k], yk, ti);
    }
    for (int k = q - 1; k >= 0; --k) {                        // L' z = y
      const double zk = __shfl(ti, k) / Ls[k * LK_PAD + k];
      if (lane == k) ti = zk;
      else if (lane < k) ti = __builtin_fma(-Ls[k * LK_PAD + lane], zk, ti);
    }
    if (lane < q) z[lane] = ti;
  }
  __syncthreads();
  if (blockIdx.x == 0 && tid < q) v[d_rows[tid]] = z[tid];
  const int64_t chunks = (mB + LK_CHUNK - 1) / LK_CHUNK;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const int64_t r = c * LK_CHUNK + tid;
    if (r < mB) {
      double acc = u[r];
      for (int j = 0; j < q; ++j) acc = __builtin_fma(-Y[r + m * j], z[j], acc);
      v[b_rows[r]] = acc;
    }
  }
}

// m = m_B + q rows in all, at least one of them a band row
inline bool lk_valid(int64_t m, int32_t q) {
  return q >= 1 && q <= LK_QMAX && m > q && m <= (int64_t)INT32_MAX - LK_CHUNK;
}

}  // namespace

extern "C" {

int ipx_link_spmm(int64_t m, int64_t n, int32_t q, const int32_t *rowptr, const int32_t *colidx,
                  const double *val, const double *Dt, const int32_t *dst_row, double *G,
                  void *stream) {
  // (any m >= 1: the product alone does not need a band row)
  if (q < 1 || q > LK_QMAX || m < 1 || m > (int64_t)INT32_MAX - LK_CHUNK || n < 1 || !rowptr ||
      !Dt || !dst_row || !G)
    return IPX_EINVAL;
  const int64_t grid = (m + LK_ROWS - 1) / LK_ROWS;
  hipLaunchKernelGGL(k_lk_spmm, dim3((unsigned)grid), dim3(IPX_BLOCK), 0, (hipStream_t)stream, m,
                     (int)q, rowptr, colidx, val, Dt, dst_row, G);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

int ipx_link_chol(int64_t m, int32_t q, const double *G, const double *part, double *K, double *L,
                  double *info, void *stream) {
  if (!lk_valid(m, q) || !G || !part || !K || !L || !info) return IPX_EINVAL;
  hipLaunchKernelGGL(k_lk_chol, dim3(1), dim3(IPX_BLOCK), 0, (hipStream_t)stream, m, (int)q,
                     ipx_border_groups(m), G, part, K, L, info);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

int ipx_link_apply(int64_t m, int32_t q, const double *Y, const double *L, const double *part,
                   const double *u, const double *w, const int32_t *b_rows, const int32_t *d_rows,
                   double *v, void *stream) {
  if (!lk_valid(m, q) || !Y || !L || !part || !u || !w || !b_rows || !d_rows || !v || v == w ||
      v == u)
    return IPX_EINVAL;
  const int64_t chunks = (m - q + LK_CHUNK - 1) / LK_CHUNK;
  const int grid = (int)(chunks < LK_APPLY_CAP ? chunks : LK_APPLY_CAP);
  hipLaunchKernelGGL(k_lk_apply, dim3(grid), dim3(IPX_BLOCK), 0, (hipStream_t)stream, m, (int)q,
                     ipx_border_groups(m), Y, L, part, u, w, b_rows, d_rows, v);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

}  // extern "C"
