// Column-pivoted Householder QR of A' for a dense row-major Jacobian A (m x n, m <= n): the
// rank-revealing half of the complete orthogonal decomposition behind DenseCODProjector
// (ipsolver/dense_cod.py), the device exit for rank-deficient dense Jacobians.
//
// Layout: csrc/denseqr.hip's.  W is the zero-padded M x N copy of A, row i = column i of A',
// everything that runs along n is coalesced, a workgroup works on a chunk of 512 columns
// (qr_common.h: the geometry, the reflector and the chunk loads / stores of both files).
//
// No row is moved.  perm[j] names the row that is pivot j, pos[i] the pivot position of row i
// (-1: none yet).  Reflector j acts on the coordinates k >= j of every row that is not a pivot
// yet: such a row keeps R(0 .. j, .) in its first j + 1 entries.  The pivot row itself is never
// written again: its entries k < j are R(k, j), R(j, j) = beta goes to diag[j], and its tail
// stays UNSCALED with 1 / (alpha - beta) in vinv[j] (the reflector is v_j = (1, tail * vinv[j])
// -- a row that other workgroups of the same launch read is not written in it).
//
// Two plain launches per step j:
//   select    every workgroup sums, in chunk order, the partial squared norms over k >= j that
//             the launch before left for every remaining row, picks the largest (ties: the
//             lowest row), applies the rank rule sqrt(norm2) > 2^-43 |R_00| (IPX_PIVOT_RTOL on R;
//             sqrt(norm2) is |R_jj| up to rounding) -- a failure sets the device words done = 1,
//             rank = j -- and leaves, for its rows on its chunk, the partial dot products
//             with the pivot row over k > j and the pivot column W[i][j].
//   reflect   sums those in chunk order, forms alpha / beta / tau with k_qr_panel's qr_dlarfg
//             (qr_common.h; a zero tail: tau = 0), applies the reflector to its remaining rows on its chunk and
//             leaves their partial squared norms over k > j.
// The norms are recomputed at every step from the values the update holds in registers anyway:
// nothing is downdated, so no cancellation safeguard is needed.  All 2 m launches are enqueued
// up front; once the rank is set each returns at its first instruction.  No workgroup waits for
// another, nothing is accumulated atomically, every sum has a fixed order.
//
// The grid is (chunks, row groups): row i belongs to group i % groups, and every partial is
// indexed by (chunk, row), so the sums do not depend on the number of groups.
#include "qr_common.h"

namespace {

constexpr int PWAVES = IPX_BLOCK / IPX_WAVE;
constexpr int PROWS = 1024;                  // rows per workgroup at most (LDS of k_qrp_reflect)
constexpr int PUNITS = 512;                  // workgroups aimed at
constexpr int PRB = 4;                       // rows a thread of k_qrp_select sums at a time

// offsets into the doubles / ints a factorization keeps (M = padded m)
struct QrpD {
  int64_t tau, diag, vinv, dn, total;
  __host__ __device__ explicit QrpD(int64_t M) { tau = 0; diag = M; vinv = 2 * M; dn = 3 * M; total = 4 * M + 8; }
};
struct QrpI {
  int64_t perm, pos, state, total;
  __host__ __device__ explicit QrpI(int64_t M) { perm = 0; pos = M; state = 2 * M; total = 2 * M + 8; }
};
struct QrpWs {
  int64_t np, dp, pv, total;
  QrpWs(int64_t M, int64_t N) {
    const int64_t nch = qr_chunks(N);
    np = 0; dp = nch * M; pv = 2 * nch * M; total = pv + M;
  }
};

int qrp_groups(int M, int nch) {
  int g = (PUNITS + nch - 1) / nch;
  if (g > M / 16) g = M / 16;
  const int least = (M + PROWS - 1) / PROWS;
  if (g < least) g = least;
  return g < 1 ? 1 : g;
}

// W (M x N) <- A zero-padded; the doubles and ints of the factorization <- their start values
__global__ void __launch_bounds__(IPX_BLOCK)
k_qrp_copy_in(int m, int n, const double *__restrict__ A, int64_t lda, double *__restrict__ W, int M,
              int N, double *__restrict__ dw, int *__restrict__ iw) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < (int64_t)M * N) {
    const int r = (int)(e / N), k = (int)(e % N);
    W[e] = (r < m && k < n) ? A[(int64_t)r * lda + k] : 0.0;
  }
  if (e < QrpD(M).total) dw[e] = 0.0;
  if (e < QrpI(M).total) iw[e] = e < 2 * (int64_t)M ? -1 : (e == 2 * (int64_t)M + 1 ? m : 0);
}

__global__ void __launch_bounds__(IPX_BLOCK)
k_qrp_select(const double *__restrict__ W, int N, int m, int M, int j, int c0, int nch,
             const double *__restrict__ np, double *__restrict__ dp, double *__restrict__ pv,
             double *__restrict__ dn, int *perm, int *pos, int *state) {
  // (the word that ends the factorization is the rank: a step returns when the rank lies before
  // it.  This launch's own verdict, rank = j, does not satisfy that test, so the waves of one
  // workgroup cannot disagree about it whenever they read the word)
  if (state[1] < j) return;
  __shared__ double s_v[PWAVES];
  __shared__ double s_i[PWAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the remaining squared norms and their largest: the same bits in every workgroup
  double best = -1.0;
  int bi = INT_MAX;
  // (PRB rows at a time: their loads are independent, each row's sum stays in chunk order)
  for (int base = tid; base < m; base += PRB * IPX_BLOCK) {
    double t[PRB];
    int ps[PRB];
#pragma unroll
    for (int q = 0; q < PRB; ++q) {
      t[q] = 0.0;
      ps[q] = pos[min(base + q * IPX_BLOCK, m - 1)];
    }
#pragma unroll 2
    for (int cc = c0; cc < nch; ++cc) {
#pragma unroll
      for (int q = 0; q < PRB; ++q) t[q] += np[(int64_t)cc * M + min(base + q * IPX_BLOCK, m - 1)];
    }
#pragma unroll
    for (int q = 0; q < PRB; ++q) {
      const int i = base + q * IPX_BLOCK;
      // (rows in increasing order: ties keep the lowest)
      if (i < m && !(ps[q] >= 0 && ps[q] < j) && t[q] > best) {
        best = t[q];
        bi = i;
      }
    }
  }
  const double wmax = ipx_wave_max(best);
  const double widx = ipx_wave_min(best == wmax ? (double)bi : (double)INT_MAX);
  if (lane == 0) {
    s_v[wave] = wmax;
    s_i[wave] = widx;
  }
  __syncthreads();
  double val = s_v[0], idx = s_i[0];
  for (int w = 1; w < PWAVES; ++w)
    if (s_v[w] > val || (s_v[w] == val && s_i[w] < idx)) {
      val = s_v[w];
      idx = s_i[w];
    }
  const bool none = !(val >= 0.0) || idx >= (double)INT_MAX;      // (no row left, or only NaNs)
  const double d = none ? 0.0 : sqrt(val);
  const double d0 = j == 0 ? d : dn[0];
  const bool fail = none || !(d > IPX_PIVOT_RTOL * d0);
  const int p = none ? 0 : (int)idx;
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
    dn[j] = d;
    if (fail) {
      state[1] = j;
      state[0] = 1;
    } else {
      perm[j] = p;
      pos[p] = j;
    }
  }
  if (fail) return;
  // the pivot row on this chunk (k > j), then the dot products of this workgroup's rows with it
  const int c = c0 + blockIdx.x;
  const int kbase = c * QR_CHUNK + lane;
  double a[QR_U];
#pragma unroll
  for (int u = 0; u < QR_U; ++u) {
    const int k = kbase + u * IPX_WAVE;
    a[u] = (k < N && k > j) ? W[(int64_t)p * N + k] : 0.0;
  }
  const int groups = gridDim.y;
  for (int li = wave; ; li += PWAVES) {
    const int i = blockIdx.y + groups * li;
    if (i >= m) break;
    const int ps = pos[i];
    if (ps >= 0 && ps < j) continue;
    double x[QR_U];
    qr_load_chunk(W + (int64_t)i * N, kbase, N, x);
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < QR_U; ++u) {
      s += a[u] * x[u];
      if (kbase + u * IPX_WAVE == j) pv[i] = x[u];
    }
    s = ipx_wave_sum(s);
    if (lane == 0) dp[(int64_t)c * M + i] = s;
  }
}

// j < 0: the squared norms of every row only (the start of the factorization)
__global__ void __launch_bounds__(IPX_BLOCK)
k_qrp_reflect(double *__restrict__ W, int N, int m, int M, int j, int c0, int nch,
              const double *__restrict__ dp, const double *__restrict__ pv, double *__restrict__ np,
              double *__restrict__ dw, const int *__restrict__ perm, const int *__restrict__ pos,
              const int *__restrict__ state) {
  if (state[1] <= j) return;
  __shared__ double s_w[PROWS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int groups = gridDim.y;
  const int c = c0 + blockIdx.x;
  const int kbase = c * QR_CHUNK + lane;
  double v[QR_U] = {};
  double tv = 0.0;
  if (j >= 0) {
    const int p = perm[j];
    double tj = 0.0;
#pragma unroll 4
    for (int cc = c0; cc < nch; ++cc) tj += dp[(int64_t)cc * M + p];
    const QrReflector h = qr_dlarfg(pv[p], tj);
    const double inv = h.inv;
    tv = h.tau;
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
      const QrpD o(M);
      dw[o.tau + j] = tv;
      dw[o.diag + j] = h.beta;
      dw[o.vinv + j] = inv;
    }
    // the coefficient of v in the update of each of this workgroup's rows
    for (int li = tid; li < PROWS; li += IPX_BLOCK) {
      const int i = blockIdx.y + groups * li;
      if (i >= m) break;
      double t = 0.0;
#pragma unroll 4
      for (int cc = c0; cc < nch; ++cc) t += dp[(int64_t)cc * M + i];
      s_w[li] = tv * (pv[i] + t * inv);
    }
    qr_reflector_chunk(W + (int64_t)p * N, kbase, j, N, inv, v);
    __syncthreads();
  }
  for (int li = wave; li < PROWS; li += PWAVES) {
    const int i = blockIdx.y + groups * li;
    if (i >= m) break;
    const int ps = pos[i];
    if (ps >= 0 && ps <= j) continue;                // (a pivot row, this step's included)
    double x[QR_U];
    qr_load_chunk(W + (int64_t)i * N, kbase, N, x);
    if (j >= 0 && tv != 0.0) {
      const double w = s_w[li];
#pragma unroll
      for (int u = 0; u < QR_U; ++u) x[u] -= w * v[u];
      qr_store_chunk(W + (int64_t)i * N, kbase, j, N, x);
    }
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < QR_U; ++u) {
      const int k = kbase + u * IPX_WAVE;
      if (k > j) s += x[u] * x[u];
    }
    s = ipx_wave_sum(s);
    if (lane == 0) np[(int64_t)c * M + i] = s;
  }
}

// perm[rank .. m) <- the rows that are no pivot, in increasing order (perm becomes a
// permutation of 0 .. m - 1).  One wave.
__global__ void __launch_bounds__(IPX_WAVE)
k_qrp_finish(int m, int M, int *__restrict__ iw) {
  const QrpI o(M);
  int *perm = iw + o.perm;
  const int *pos = iw + o.pos;
  const int lane = threadIdx.x;
  int count = iw[o.state + 1];
  for (int base = 0; base < m; base += IPX_WAVE) {
    const int i = base + lane;
    const bool free_row = i < m && pos[i] < 0;
    const unsigned long long mask = __ballot(free_row);
    if (free_row) perm[count + __popcll(mask & ((1ull << lane) - 1ull))] = i;
    count += __popcll(mask);
  }
}

// Vp (Mr x N) <- the first r reflectors in pivot order, in the form of ipx_qr_factor's W
// (row jj = (0 .. 0, 1, tail of row perm[jj] * vinv[jj]); zero rows on the padding);
// taup (Mr) <- their tau, zero on the padding
__global__ void __launch_bounds__(IPX_BLOCK)
k_qrp_reflectors(int r, int Mr, int N, int M, const double *__restrict__ W,
                 const double *__restrict__ dw, const int *__restrict__ iw, double *__restrict__ Vp,
                 double *__restrict__ taup) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)Mr * N) return;
  const QrpD o(M);
  const int jj = (int)(e / N), k = (int)(e % N);
  double val = 0.0;
  if (jj < r) {
    if (k == jj) val = 1.0;
    else if (k > jj) val = W[(int64_t)iw[jj] * N + k] * dw[o.vinv + jj];
  }
  Vp[e] = val;
  if (k == 0) taup[jj] = jj < r ? dw[o.tau + jj] : 0.0;
}

// T (r x m, row-major, leading dimension ldt) <- R[:r, :] in pivot order: T[jj][cpos] = R(jj,
// cpos) = entry jj of row perm[cpos] (the diagonal from diag), exactly zero below the diagonal
__global__ void __launch_bounds__(IPX_BLOCK)
k_qrp_write_t(int r, int m, int N, int M, const double *__restrict__ W, const double *__restrict__ dw,
              const int *__restrict__ iw, double *__restrict__ T, int64_t ldt) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)r * m) return;
  const QrpD o(M);
  const int jj = (int)(e / m), cpos = (int)(e % m);
  double val = 0.0;
  if (cpos == jj) val = dw[o.diag + jj];
  else if (cpos > jj) val = W[(int64_t)iw[cpos] * N + jj];
  T[(int64_t)jj * ldt + cpos] = val;
}

// out[row][perm[cpos]] = in[row][cpos], cpos < m: the permutation folded into the columns
__global__ void __launch_bounds__(IPX_BLOCK)
k_qrp_fold_columns(int rows, int m, int64_t ld, const double *__restrict__ in,
                   const int *__restrict__ perm, double *__restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)rows * m) return;
  const int row = (int)(e / m), cpos = (int)(e % m);
  out[(int64_t)row * ld + perm[cpos]] = in[(int64_t)row * ld + cpos];
}

}  // namespace

extern "C" {

int64_t ipx_qrp_ws_doubles(int64_t m, int64_t n) {
  if (m < 1 || n < m) return 0;
  return QrpWs(ipx_dense_padded(m), ipx_qr_padded_cols(n)).total;
}
int64_t ipx_qrp_info_doubles(int64_t m) { return m < 1 ? 0 : QrpD(ipx_dense_padded(m)).total; }
int64_t ipx_qrp_info_ints(int64_t m) { return m < 1 ? 0 : QrpI(ipx_dense_padded(m)).total; }

// A' P = Q [R11 R12] for the row-major A (m x n, m <= n, leading dimension lda), see the head of
// this file.  M = ipx_dense_padded(m), N = ipx_qr_padded_cols(n).  On return: W (M x N) the
// reflected rows; dw (ipx_qrp_info_doubles(m)) = tau (M) | diag R (M) | 1 / (alpha - beta) (M)
// | the pivot norms sqrt(norm2) of the steps taken, the rejected one included (M + 8);
// iw (ipx_qrp_info_ints(m)) = perm (M; a permutation of 0 .. m - 1) | pos (M) | done, rank.
// ws: ipx_qrp_ws_doubles(m, n) doubles.  2 m + 3 launches, none of them waits for the host.
int ipx_qrp_factor(int64_t m, int64_t n, const double *A, int64_t lda, double *W, double *dw,
                   int32_t *iw, double *ws, void *stream) {
  if (m < 1 || n < m || !A || lda < n || !W || !dw || !iw || !ws) return IPX_EINVAL;
  if (n > (1 << 30)) return IPX_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int M = (int)ipx_dense_padded(m), N = (int)ipx_qr_padded_cols(n);
  const int nch = qr_chunks(N);
  const int groups = qrp_groups(M, nch);
  const QrpWs o(M, N);
  const QrpD od(M);
  const QrpI oi(M);
  int *perm = iw + oi.perm, *pos = iw + oi.pos, *state = iw + oi.state;
  hipLaunchKernelGGL(k_qrp_copy_in, dim3(qr_grid((int64_t)M * N)), dim3(IPX_BLOCK), 0, st, (int)m,
                     (int)n, A, lda, W, M, N, dw, (int *)iw);
  IPX_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_qrp_reflect, dim3(nch, groups), dim3(IPX_BLOCK), 0, st, W, N, (int)m, M, -1,
                     0, nch, (const double *)(ws + o.dp), (const double *)(ws + o.pv), ws + o.np, dw,
                     (const int *)perm, (const int *)pos, (const int *)state);
  IPX_CHECK_LAUNCH();
  for (int j = 0; j < (int)m; ++j) {
    const int c0 = j / QR_CHUNK;
    const dim3 grid(nch - c0, groups), block(IPX_BLOCK);
    hipLaunchKernelGGL(k_qrp_select, grid, block, 0, st, (const double *)W, N, (int)m, M, j, c0, nch,
                       (const double *)(ws + o.np), ws + o.dp, ws + o.pv, dw + od.dn, perm, pos,
                       state);
    IPX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_qrp_reflect, grid, block, 0, st, W, N, (int)m, M, j, c0, nch,
                       (const double *)(ws + o.dp), (const double *)(ws + o.pv), ws + o.np, dw,
                       (const int *)perm, (const int *)pos, (const int *)state);
    IPX_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_qrp_finish, dim3(1), dim3(IPX_WAVE), 0, st, (int)m, M, (int *)iw);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

// The first r reflectors of ipx_qrp_factor in pivot order, as ipx_qr_wy / ipx_qr_form_q take
// them: Vp (Mr x N, Mr = ipx_dense_padded(r)), taup (Mr).
int ipx_qrp_reflectors(int64_t m, int64_t n, int64_t r, const double *W, const double *dw,
                       const int32_t *iw, double *Vp, double *taup, void *stream) {
  if (m < 1 || n < m || r < 1 || r > m || !W || !dw || !iw || !Vp || !taup) return IPX_EINVAL;
  const int M = (int)ipx_dense_padded(m), N = (int)ipx_qr_padded_cols(n);
  const int Mr = (int)ipx_dense_padded(r);
  hipLaunchKernelGGL(k_qrp_reflectors, dim3(qr_grid((int64_t)Mr * N)), dim3(IPX_BLOCK), 0,
                     (hipStream_t)stream, (int)r, Mr, N, M, W, dw, (const int *)iw, Vp, taup);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

// T (r x m, row-major, leading dimension ldt >= m) <- [R11 R12], columns in pivot order
int ipx_qrp_write_t(int64_t m, int64_t n, int64_t r, const double *W, const double *dw,
                    const int32_t *iw, double *T, int64_t ldt, void *stream) {
  if (m < 1 || n < m || r < 1 || r > m || !W || !dw || !iw || !T || ldt < m) return IPX_EINVAL;
  const int M = (int)ipx_dense_padded(m), N = (int)ipx_qr_padded_cols(n);
  hipLaunchKernelGGL(k_qrp_write_t, dim3(qr_grid(r * m)), dim3(IPX_BLOCK), 0, (hipStream_t)stream,
                     (int)r, (int)m, N, M, W, dw, (const int *)iw, T, ldt);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

// out[row][perm[c]] = in[row][c] for row < rows, c < m (leading dimension ld of both; out's
// other entries are left as they are): Q2' P' from Q2'
int ipx_qrp_fold_columns(int64_t rows, int64_t m, int64_t ld, const double *in, const int32_t *perm,
                         double *out, void *stream) {
  if (rows < 1 || m < 1 || ld < m || !in || !perm || !out || in == out) return IPX_EINVAL;
  hipLaunchKernelGGL(k_qrp_fold_columns, dim3(qr_grid(rows * m)), dim3(IPX_BLOCK), 0,
                     (hipStream_t)stream, (int)rows, (int)m, ld, in, (const int *)perm, out);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

}  // extern "C"
