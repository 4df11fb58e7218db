// Blocked Householder QR of A' for a dense row-major Jacobian A (m x n, m <= n): the
// reference's dense factorization (projections.py:175-233, LAPACK QR of A.T) on the device,
// unpivoted.  Its operators lose cond(A) eps where Gram + Cholesky (csrc/dense.hip) loses
// cond(A)^2 eps.
//
// Layout.  Column j of A' is the contiguous row j of A, so everything that runs along n --
// norms, dot products, axpys -- is coalesced.  The factorization works on a zero-padded copy W
// (M x N, M = m rounded up to 64, N = n rounded up to 64): reflector j lives in row j,
// v_j = (0 .. 0, 1, W[j][j+1 .. N)), and R'(i, k) = R(k, i) is what row i holds in its first
// i + 1 entries.  Zero padding is exact: a padded column of A' is a zero column (tau = 0), a
// padded row of A' a zero row of every reflector.
//
// Right-looking, panels of 64 rows (the MFMA tile of mfma_tile.h):
//   panel     one plain launch per reflector (k_qr_panel), a workgroup per chunk of 512 columns
//             of the panel's rows: it sums -- in chunk order -- the partial dot products the
//             launch before it left, forms alpha / beta / tau from them, applies the reflector
//             to the panel rows behind it on its chunk, and leaves the partial dot products of
//             the next row.  No workgroup waits for another; nothing is accumulated atomically.
//   extract   R' of the panel's rows goes to L (M x M, lower triangular), the rows become the
//             clean unit-trapezoidal V the tile products want (k_qr_extract).
//   compact   S = V V' (split-K MFMA tiles, fixed-order reduce), T from tau and S by the dlarft
//   WY        recurrence in one workgroup (k_qr_tform).
//   trailing  X <- X - ((X V) T) V' for the rows X behind the panel: X V as split-K MFMA tiles
//             (the same launch as S: the panel is its tile 0), W T, and the rank-64 update.
// Q is formed explicitly as Q' (M x N, row r = column r of Q) by backward accumulation with
// the same three block kernels (dorgqr), T transposed.  R^-1 comes from the recursive-doubling
// triangular inverse of csrc/dense.hip (ipx_trtri_lower) on a copy of L.
//
// Launches per factorization, nt = M / 64 panels: m + nt (panel) + nt (extract) + 3 nt (S, T)
// + 2 (nt - 1) (trailing) + 3 (set-up, pivot ratio) for ipx_qr_factor, 4 nt + 1 for
// ipx_qr_form_q.  Norms are plain sums of squares: entries beyond about 1e+-150 are out of
// scope.
// The chunk geometry, the reflector (dlarfg) and the guarded chunk loads / stores of k_qr_panel
// are qr_common.h's, shared with the pivoted factorization of csrc/denseqrp.hip.
#include "mfma_tile.h"
#include "qr_common.h"

namespace {

constexpr int QB = GT;           // panel width = tile edge
constexpr int QTILE = QB * QB;
constexpr int QSPLIT_MAX = 16;
constexpr int QUNITS = 256;      // split-K units aimed at (one per CU)

// W (M x N) <- A zero-padded; rn2[r] = sum_k A[r][k]^2 (lane-strided partial sums, then the
// wave butterfly: a fixed order).  One wave per row.
__global__ void __launch_bounds__(IPX_BLOCK)
k_qr_copy_in(int m, int n, const double *__restrict__ A, int64_t lda, double *__restrict__ W,
             int M, int N, double *__restrict__ rn2) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * (IPX_BLOCK / IPX_WAVE) + wave;
  if (r >= M) return;
  double s = 0.0;
  for (int k = lane; k < N; k += IPX_WAVE) {
    const double v = (r < m && k < n) ? A[(int64_t)r * lda + k] : 0.0;
    W[(int64_t)r * N + k] = v;
    s += v * v;
  }
  s = ipx_wave_sum(s);
  if (lane == 0) rn2[r] = s;
}

// QT (M x N) <- the first m columns of the identity, transposed
__global__ void __launch_bounds__(IPX_BLOCK)
k_qr_eye(int m, int M, int N, double *__restrict__ QT) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)M * N) return;
  const int r = (int)(e / N), k = (int)(e % N);
  QT[e] = (r == k && r < m) ? 1.0 : 0.0;
}

// L (M x M) <- 0 with ones on the padded part of the diagonal; tau (M) <- 0
__global__ void __launch_bounds__(IPX_BLOCK)
k_qr_init(int m, int M, double *__restrict__ L, double *__restrict__ tau) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)M * M) return;
  const int r = (int)(e / M), k = (int)(e % M);
  L[e] = (r == k && r >= m) ? 1.0 : 0.0;
  if (e < M) tau[e] = 0.0;
}

// One step of a panel [j0, j0 + jb).  With j >= 0: reflector j from the partial dot products
// `pin` (chunk c at pin[64 c ..], entry i - j0: the sum over the chunk's k > j of
// W[j][k] W[i][k]) and the pivot column pvin[i - j0] = W[i][j], applied to rows (j, j0 + jb) on
// this workgroup's chunk; row j becomes (beta, v).  With jn >= 0: the same two quantities of
// row jn, AFTER this update, into pout / pvout.  Chunks c0, c0 + 1, ...: blockIdx.x.
__global__ void __launch_bounds__(IPX_BLOCK)
k_qr_panel(double *__restrict__ W, int N, int j0, int jb, int j, int jn, int c0, int nchunks,
           const double *__restrict__ pin, const double *__restrict__ pvin,
           double *__restrict__ pout, double *__restrict__ pvout, double *__restrict__ tau) {
  __shared__ double s_t[QB];
  __shared__ double s_p[QB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = c0 + blockIdx.x;
  const int kbase = c * QR_CHUNK + lane;
  const int j1 = j0 + jb;
  double tj = 0.0;
  QrReflector h{0.0, 0.0, 0.0};
  if (j >= 0) {
    if (tid < QB) {
      double t = 0.0;
      if (j0 + tid >= j && j0 + tid < j1)
        for (int cc = c0; cc < nchunks; ++cc) t += pin[cc * QB + tid];
      s_t[tid] = t;
      s_p[tid] = (j0 + tid >= j && j0 + tid < j1) ? pvin[tid] : 0.0;
    }
    __syncthreads();
    tj = s_t[j - j0];
    h = qr_dlarfg(s_p[j - j0], tj);
    if (blockIdx.x == 0 && tid == 0) tau[j] = h.tau;
  }
  const double beta = h.beta, tv = h.tau, inv = h.inv;
  // everything other waves are about to overwrite is read first: row j (the reflector), row jn
  double v[QR_U] = {}, a[QR_U] = {};
  if (j >= 0) qr_reflector_chunk(W + (int64_t)j * N, kbase, j, N, inv, v);
  if (jn >= 0) qr_load_chunk(W + (int64_t)jn * N, kbase, N, a);
  __syncthreads();
  if (j >= 0 && wave == 0) {
#pragma unroll
    for (int u = 0; u < QR_U; ++u) {
      const int k = kbase + u * IPX_WAVE;
      if (k < N && k >= j && tj != 0.0) W[(int64_t)j * N + k] = k == j ? beta : v[u];
    }
  }
  // rows j + 1 + wave, + 4, ...: update, store, and (jn >= 0) the dot with the updated row jn
  const int first = (j >= 0 ? j + 1 : jn) + wave;
  if (j >= 0 && jn >= 0) {
    const double w = tv * (s_p[jn - j0] + s_t[jn - j0] * inv);
#pragma unroll
    for (int u = 0; u < QR_U; ++u) a[u] -= w * v[u];
  }
  // (a wave's rows are a chain of load - update - store - reduce steps: the loads of its next
  // row are issued before the arithmetic of the current one, which the compiler cannot do
  // across the stores)
  double xn[QR_U] = {};
  if (first < j1 && first != jn) qr_load_chunk(W + (int64_t)first * N, kbase, N, xn);
  for (int i = first; i < j1; i += IPX_BLOCK / IPX_WAVE) {
    double x[QR_U];
#pragma unroll
    for (int u = 0; u < QR_U; ++u) x[u] = i == jn ? a[u] : xn[u];
    const int inext = i + IPX_BLOCK / IPX_WAVE;      // (never row jn: that is the first row)
    if (inext < j1) qr_load_chunk(W + (int64_t)inext * N, kbase, N, xn);
    if (i != jn) {
      if (j >= 0) {
        const double w = tv * (s_p[i - j0] + s_t[i - j0] * inv);
#pragma unroll
        for (int u = 0; u < QR_U; ++u) x[u] -= w * v[u];
      }
    }
    if (j >= 0 && tv != 0.0) qr_store_chunk(W + (int64_t)i * N, kbase, j, N, x);
    if (jn >= 0) {
      double s = 0.0;
#pragma unroll
      for (int u = 0; u < QR_U; ++u) {
        const int k = kbase + u * IPX_WAVE;
        if (k > jn) s += a[u] * x[u];
        if (k == jn) pvout[i - j0] = x[u];
      }
      s = ipx_wave_sum(s);
      if (lane == 0) pout[c * QB + (i - j0)] = s;
    }
  }
}

// Rows [j0, j0 + jb): L[i][k] <- W[i][k] for k <= i (= R(k, i)), W[i][k] <- (k == i).
__global__ void __launch_bounds__(IPX_BLOCK)
k_qr_extract(double *__restrict__ W, int N, int j0, double *__restrict__ L, int M) {
  const int i = j0 + blockIdx.x;
  for (int k = threadIdx.x; k <= i; k += IPX_BLOCK) {
    L[(int64_t)i * M + k] = W[(int64_t)i * N + k];
    W[(int64_t)i * N + k] = (k == i) ? 1.0 : 0.0;
  }
}

// Partial tiles of X V' over columns [j0, N) cut into `splits` parts: X = `tiles` row tiles
// of 64 rows (leading dimension ldx) from X0, V = the 64 panel rows (leading dimension ldv)
// from V0; both pointers at column j0.  ws[(split * tiles + tile) * 4096 + 64 row + col].
__global__ void __launch_bounds__(IPX_BLOCK)
k_qr_xv(const double *__restrict__ X0, int64_t ldx, const double *__restrict__ V0, int64_t ldv,
        int K, int tiles, int splits, double *__restrict__ ws) {
  __shared__ __attribute__((aligned(16))) double sA[GPANEL];
  __shared__ __attribute__((aligned(16))) double sB[GPANEL];
  const int tile = (int)blockIdx.x % tiles, split = (int)blockIdx.x / tiles;
  const int nchunk = K / GK;
  const int kbeg = (int)((int64_t)split * nchunk / splits) * GK;
  const int kend = (int)((int64_t)(split + 1) * nchunk / splits) * GK;
  const Opnd Pn{X0 + (int64_t)tile * QB * ldx + kbeg, ldx, 1};
  const Opnd Qn{V0 + kbeg, ldv, 1};
  v4d acc[2][2];
  tile_pqt(Pn, Qn, kend - kbeg, acc, sA, sB);
  double *out = ws + ((int64_t)split * tiles + tile) * QTILE;
  IPX_TILE_FOREACH(acc, row, col, val, out[row * QB + col] = val);
}

// out[tile] = sum over the splits, in split order
__global__ void __launch_bounds__(IPX_BLOCK)
k_qr_reduce(const double *__restrict__ ws, int tiles, int splits, double *__restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t tot = (int64_t)tiles * QTILE;
  if (e >= tot) return;
  double v = 0.0;
  for (int s = 0; s < splits; ++s) v += ws[(int64_t)s * tot + e];
  out[e] = v;
}

// T (64 x 64, upper triangular) of the compact WY form from S = V V' and tau (dlarft, forward,
// columnwise): T[c][c] = tau_c, T[r][c] = -tau_c sum_{q = r}^{c-1} T[r][q] S[q][c].  One wave.
__global__ void __launch_bounds__(IPX_WAVE)
k_qr_tform(const double *__restrict__ S, const double *__restrict__ tau, double *__restrict__ T) {
  __shared__ double Ts[QB][QB + 1];
  __shared__ double Ss[QB][QB + 1];
  const int r = threadIdx.x;
  for (int q = 0; q < QB; ++q) {
    Ss[q][r] = S[q * QB + r];
    Ts[q][r] = 0.0;
  }
  __syncthreads();
  for (int c = 0; c < QB; ++c) {
    const double tc = tau[c];
    double t = 0.0;
    if (r < c) {
      double s = 0.0;
      for (int q = r; q < c; ++q) s += Ts[r][q] * Ss[q][c];
      t = -tc * s;
    } else if (r == c) {
      t = tc;
    }
    Ts[r][c] = t;
    __syncthreads();
  }
  for (int q = 0; q < QB; ++q) T[q * QB + r] = Ts[q][r];
}

// wt[tile] = wk[tile] T (TRANS = 0) or wk[tile] T' (TRANS = 1)
template <int TRANS>
__global__ void __launch_bounds__(IPX_BLOCK)
k_qr_wt(const double *__restrict__ wk, const double *__restrict__ T, double *__restrict__ wt) {
  __shared__ __attribute__((aligned(16))) double sA[GPANEL];
  __shared__ __attribute__((aligned(16))) double sB[GPANEL];
  const Opnd Pn{wk + (int64_t)blockIdx.x * QTILE, QB, 1};
  const Opnd Qn{T, TRANS ? QB : 1, TRANS ? 1 : QB};       // element (col, k) of the product's Q
  v4d acc[2][2];
  tile_pqt(Pn, Qn, QB, acc, sA, sB);
  double *out = wt + (int64_t)blockIdx.x * QTILE;
  IPX_TILE_FOREACH(acc, row, col, val, out[row * QB + col] = val);
}

// X[tile ty][column tile tx] -= wt[ty] V[:, tx]   (rank 64); X0 / V0 at column j0
__global__ void __launch_bounds__(IPX_BLOCK)
k_qr_update(double *__restrict__ X0, int64_t ldx, const double *__restrict__ V0, int64_t ldv,
            const double *__restrict__ wt) {
  __shared__ __attribute__((aligned(16))) double sA[GPANEL];
  __shared__ __attribute__((aligned(16))) double sB[GPANEL];
  const int tx = blockIdx.x, ty = blockIdx.y;
  const Opnd Pn{wt + (int64_t)ty * QTILE, QB, 1};
  const Opnd Qn{V0 + (int64_t)tx * QB, 1, ldv};
  v4d acc[2][2];
  tile_pqt(Pn, Qn, QB, acc, sA, sB);
  double *x = X0 + (int64_t)ty * QB * ldx + (int64_t)tx * QB;
  IPX_TILE_FOREACH(acc, row, col, val, x[(int64_t)row * ldx + col] -= val);
}

// out[0] = min_j |R_jj| / ||row j of A||  (a zero row: 0).  One workgroup; a minimum does not
// depend on the order it is taken in.
__global__ void __launch_bounds__(IPX_BLOCK)
k_qr_ratio(int m, int M, const double *__restrict__ L, const double *__restrict__ rn2,
           double *__restrict__ out) {
  __shared__ double lds[IPX_BLOCK / IPX_WAVE];
  double r = __builtin_inf();
  for (int j = threadIdx.x; j < m; j += IPX_BLOCK) {
    const double d = fabs(L[(int64_t)j * M + j]), s = rn2[j];
    const double q = (s > 0.0 && d == d) ? d / sqrt(s) : 0.0;
    r = fmin(r, q);
  }
  r = ipx_block_reduce<IPX_MIN>(r, lds);
  if (threadIdx.x == 0) out[0] = r;
}

// strict upper triangle of G (M x M) <- 0
__global__ void __launch_bounds__(IPX_BLOCK)
k_qr_clear_upper(int M, double *__restrict__ G) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)M * M) return;
  if ((int)(e % M) > (int)(e / M)) G[e] = 0.0;
}

int qr_splits(int tiles, int K) {
  int s = QUNITS / tiles;
  if (s > QSPLIT_MAX) s = QSPLIT_MAX;
  if (s > K / 128) s = K / 128;
  return s < 1 ? 1 : s;
}

// workspace offsets (doubles)
struct QrWs {
  int64_t part, piv, xv, wk, wt, total;
  QrWs(int64_t M, int64_t N) {
    const int64_t nt = M / QB, nch = qr_chunks(N);
    part = 0;
    piv = part + 2 * nch * QB;
    xv = piv + 2 * QB;
    wk = xv + (QUNITS + nt) * QTILE;
    wt = wk + nt * QTILE;
    total = wt + nt * QTILE;
  }
};

// wk[0 .. tiles) <- X V' over columns [j0, N) (X: `tiles` row tiles from X0, V: the panel at V0)
int qr_xv(const double *X0, int64_t ldx, const double *V0, int64_t ldv, int K, int tiles,
          double *ws, const QrWs &o, hipStream_t st) {
  const int splits = qr_splits(tiles, K);
  hipLaunchKernelGGL(k_qr_xv, dim3(tiles * splits), dim3(IPX_BLOCK), 0, st, X0, ldx, V0, ldv, K,
                     tiles, splits, ws + o.xv);
  IPX_CHECK_LAUNCH();
  const int64_t tot = (int64_t)tiles * QTILE;
  hipLaunchKernelGGL(k_qr_reduce, dim3(qr_grid(tot)),
                     dim3(IPX_BLOCK), 0, st, ws + o.xv, tiles, splits, ws + o.wk);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

// The compact WY factor of the panel at row / column j0 of the reflectors W (rows in the clean
// unit-trapezoidal form): wk[0 .. tiles) <- X V' for the `tiles` row tiles from the panel down
// (tile 0 is S = V V'), Tp <- T from tau and S.  Three launches.
int qr_wy_panel(const double *W, int N, int j0, int tiles, const double *tau, double *Tp, double *ws,
                const QrWs &o, hipStream_t st) {
  const double *V0 = W + (int64_t)j0 * N + j0;
  const int rc = qr_xv(V0, N, V0, N, N - j0, tiles, ws, o, st);
  if (rc != IPX_OK) return rc;
  hipLaunchKernelGGL(k_qr_tform, dim3(1), dim3(IPX_WAVE), 0, st, (const double *)(ws + o.wk),
                     (const double *)(tau + j0), Tp);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

}  // namespace

extern "C" {

int64_t ipx_qr_padded_cols(int64_t n) { return ((n + QB - 1) / QB) * QB; }

int64_t ipx_qr_ws_doubles(int64_t m, int64_t n) {
  if (m < 1 || n < m) return 0;
  return QrWs(ipx_dense_padded(m), ipx_qr_padded_cols(n)).total;
}

// A' = Q R for the row-major A (m x n, m <= n, leading dimension lda).  M = ipx_dense_padded(m),
// N = ipx_qr_padded_cols(n).  On return: W (M x N) the reflectors, row j = v_j with its unit
// entry; L (M x M) = R' (lower triangular, identity on the padding); T (M / 64 tiles of 64 x 64)
// the compact WY factors; tau (M); info[0] = min_j |R_jj| / ||row j of A||, info[1 .. M] = the
// squared row norms of A.  ws: ipx_qr_ws_doubles(m, n) doubles.
int ipx_qr_factor(int64_t m, int64_t n, const double *A, int64_t lda, double *W, double *L,
                  double *T, double *tau, double *info, double *ws, void *stream) {
  if (m < 1 || n < m || !A || lda < n || !W || !L || !T || !tau || !info || !ws) return IPX_EINVAL;
  if (n > (1 << 30)) return IPX_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int M = (int)ipx_dense_padded(m), N = (int)ipx_qr_padded_cols(n);
  const int nt = M / QB, nch = qr_chunks(N);
  const QrWs o(M, N);
  const int wpb = IPX_BLOCK / IPX_WAVE;
  hipLaunchKernelGGL(k_qr_copy_in, dim3((M + wpb - 1) / wpb), dim3(IPX_BLOCK), 0, st, (int)m,
                     (int)n, A, lda, W, M, N, info + 1);
  IPX_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_qr_init, dim3(qr_grid((int64_t)M * M)),
                     dim3(IPX_BLOCK), 0, st, (int)m, M, L, tau);
  IPX_CHECK_LAUNCH();
  for (int p = 0; p < nt; ++p) {
    const int j0 = p * QB;
    const int jb = (int)m - j0 < QB ? (int)m - j0 : QB;
    if (jb > 0) {
      const int c0 = j0 / QR_CHUNK;
      const dim3 grid(nch - c0), block(IPX_BLOCK);
      double *part[2] = {ws + o.part, ws + o.part + (int64_t)nch * QB};
      double *piv[2] = {ws + o.piv, ws + o.piv + QB};
      hipLaunchKernelGGL(k_qr_panel, grid, block, 0, st, W, N, j0, jb, -1, j0, c0, nch,
                         (const double *)nullptr, (const double *)nullptr, part[0], piv[0], tau);
      IPX_CHECK_LAUNCH();
      for (int j = j0; j < j0 + jb; ++j) {
        const int in = (j - j0) & 1;
        const int jn = j + 1 < j0 + jb ? j + 1 : -1;
        hipLaunchKernelGGL(k_qr_panel, grid, block, 0, st, W, N, j0, jb, j, jn, c0, nch,
                           (const double *)part[in], (const double *)piv[in], part[1 - in],
                           piv[1 - in], tau);
        IPX_CHECK_LAUNCH();
      }
      hipLaunchKernelGGL(k_qr_extract, dim3(jb), dim3(IPX_BLOCK), 0, st, W, N, j0, L, M);
      IPX_CHECK_LAUNCH();
    }
    // S = V V' (tile 0) and X V' for the rows behind the panel in one split-K launch
    const int tiles = nt - p, K = N - j0;
    const double *V0 = W + (int64_t)j0 * N + j0;
    int rc = qr_wy_panel(W, N, j0, tiles, tau, T + (int64_t)p * QTILE, ws, o, st);
    if (rc != IPX_OK) return rc;
    if (tiles > 1) {
      hipLaunchKernelGGL(k_qr_wt<0>, dim3(tiles - 1), dim3(IPX_BLOCK), 0, st,
                         (const double *)(ws + o.wk + QTILE),
                         (const double *)(T + (int64_t)p * QTILE), ws + o.wt);
      IPX_CHECK_LAUNCH();
      hipLaunchKernelGGL(k_qr_update, dim3(K / QB, tiles - 1), dim3(IPX_BLOCK), 0, st,
                         W + (int64_t)(j0 + QB) * N + j0, (int64_t)N, V0, (int64_t)N,
                         (const double *)(ws + o.wt));
      IPX_CHECK_LAUNCH();
    }
  }
  hipLaunchKernelGGL(k_qr_ratio, dim3(1), dim3(IPX_BLOCK), 0, st, (int)m, M, (const double *)L,
                     (const double *)(info + 1), info);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

// T (M / 64 tiles) <- the compact WY factors of reflectors that were not made by ipx_qr_factor
// (the pivoted factorization of csrc/denseqrp.hip): W (M x N) in ipx_qr_factor's form, tau (M).
// 3 M / 64 launches.
int ipx_qr_wy(int64_t m, int64_t n, const double *W, const double *tau, double *T, double *ws,
              void *stream) {
  if (m < 1 || n < m || !W || !tau || !T || !ws) return IPX_EINVAL;
  const int M = (int)ipx_dense_padded(m), N = (int)ipx_qr_padded_cols(n);
  const QrWs o(M, N);
  for (int p = 0; p < M / QB; ++p) {
    const int rc = qr_wy_panel(W, N, p * QB, 1, tau, T + (int64_t)p * QTILE, ws, o,
                               (hipStream_t)stream);
    if (rc != IPX_OK) return rc;
  }
  return IPX_OK;
}

// QT (M x N) <- Q' (row r = column r of the n x m factor Q; zero on the padding) from the
// reflectors W and the WY factors T of ipx_qr_factor, by backward accumulation.
int ipx_qr_form_q(int64_t m, int64_t n, const double *W, const double *T, double *QT, double *ws,
                  void *stream) {
  if (m < 1 || n < m || !W || !T || !QT || !ws) return IPX_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int M = (int)ipx_dense_padded(m), N = (int)ipx_qr_padded_cols(n);
  const int nt = M / QB;
  const QrWs o(M, N);
  hipLaunchKernelGGL(k_qr_eye, dim3(qr_grid((int64_t)M * N)),
                     dim3(IPX_BLOCK), 0, st, (int)m, M, N, QT);
  IPX_CHECK_LAUNCH();
  for (int p = nt - 1; p >= 0; --p) {
    const int j0 = p * QB, tiles = nt - p, K = N - j0;
    const double *V0 = W + (int64_t)j0 * N + j0;
    double *X0 = QT + (int64_t)j0 * N + j0;
    int rc = qr_xv(X0, N, V0, N, K, tiles, ws, o, st);
    if (rc != IPX_OK) return rc;
    hipLaunchKernelGGL(k_qr_wt<1>, dim3(tiles), dim3(IPX_BLOCK), 0, st,
                       (const double *)(ws + o.wk), T + (int64_t)p * QTILE, ws + o.wt);
    IPX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_qr_update, dim3(K / QB, tiles), dim3(IPX_BLOCK), 0, st, X0, (int64_t)N,
                       V0, (int64_t)N, (const double *)(ws + o.wt));
    IPX_CHECK_LAUNCH();
  }
  return IPX_OK;
}

// Linv (M x M) <- L^-1 for the lower triangular L of ipx_qr_factor (= R^-T; its transpose is
// R^-1), strict upper triangle exactly zero.  L is left as it is.
int ipx_qr_tri_inverse(int64_t M, const double *L, double *Linv, void *stream) {
  if (M < QB || M % QB || !L || !Linv) return IPX_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemcpyAsync(Linv, L, sizeof(double) * M * M, hipMemcpyDeviceToDevice, st) != hipSuccess)
    return IPX_ELAUNCH;
  const int rc = ipx_trtri_lower(M, Linv, stream);
  if (rc != IPX_OK) return rc;
  hipLaunchKernelGGL(k_qr_clear_upper, dim3(qr_grid(M * M)),
                     dim3(IPX_BLOCK), 0, st, (int)M, Linv);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

}  // extern "C"
