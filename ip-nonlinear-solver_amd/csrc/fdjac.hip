// Sparse finite-difference constraint Jacobians (Curtis, Powell & Reid 1974; the reference's
// _numdiff.py:15-103 steps and bounds, :484-561 grouped differences) on a fixed CSR pattern.
//
//   ipx_fd_steps      h and the one-sided flags of every variable            (elementwise)
//   ipx_fd_perturb    the perturbed point(s) of ONE group + dx of its members (elementwise)
//   ipx_fd_assemble   val[k] = df / dx[col[k]] for every stored entry, in CSR order over the
//                     pattern's SpMV row tiles: one launch per Jacobian (or per chunk of groups)
//   ipx_fd_assemble_sym  the same for a Hessian (the Jacobian of a gradient) on a symmetric
//                     pattern: val[slot[k]] (+)= 0.5 (q_ij + q_ji), exactly symmetric
//
// The per-element arithmetic is three __host__ __device__ routines (fd_step, fd_perturb_one,
// fd_quotient): the kernels and the *_host entries run the same operations in the same order,
// one rounding each (-ffp-contract=off), which is the reference's numpy expression evaluated
// per element -- the values are its bits, and CPU tests pin them.
//
// HBM bytes per launch (algorithmic): steps 8n (x0) [+ 16n bounds] + 9n out; perturb 4n + 8n +
// 8n + n in, 8n or 16n out + 8 per member; assemble 4 nnz (col) + 8 nnz (val) + per entry the
// gathers groups / dx / flag by column and f0 / F1 [/ F2] by (group, row) -- 8 to 24 B each, served
// by L2 where neighbouring entries share a column or a row.
#include "ipx_common.h"

namespace {

enum { FD_2POINT = 0, FD_3POINT = 1, FD_CS = 2 };

// np.maximum / np.minimum (a NaN operand wins; fmax / fmin would drop it)
__host__ __device__ inline double fd_npmax(double a, double b) {
  return (a != a) ? a : ((b != b) ? b : (a > b ? a : b));
}
__host__ __device__ inline double fd_npmin(double a, double b) {
  return (a != a) ? a : ((b != b) ? b : (a < b ? a : b));
}
__host__ __device__ inline double fd_abs(double a) { return a < 0.0 ? -a : (a == 0.0 ? 0.0 : a); }

// _compute_absolute_step + _adjust_scheme_to_bounds(num_steps = 1) for one variable.
__host__ __device__ inline void fd_step(int method, double rel, double x0, double lb, double ub,
                                        double *h_out, unsigned char *one_sided_out) {
  const double sign = (x0 >= 0.0) ? 1.0 : -1.0;
  double h = (rel * sign) * fd_npmax(1.0, fd_abs(x0));
  if (method == FD_CS) {
    *h_out = h;
    *one_sided_out = 0;
    return;
  }
  const double lower_dist = x0 - lb, upper_dist = ub - x0;
  if (method == FD_2POINT) {                       // scheme '1-sided'
    const double h_total = h * 1.0;
    const double x = x0 + h_total;
    const bool violated = (x < lb) || (x > ub);
    const bool fitting = fd_abs(h_total) <= fd_npmax(lower_dist, upper_dist);
    double ha = h;
    if (violated && fitting) ha = ha * -1.0;
    if ((upper_dist >= lower_dist) && !fitting) ha = upper_dist / 1.0;
    if ((upper_dist < lower_dist) && !fitting) ha = -lower_dist / 1.0;
    *h_out = ha;
    *one_sided_out = 1;
    return;
  }
  h = fd_abs(h);                                   // scheme '2-sided'
  const double h_total = h * 1.0;
  const bool central = (lower_dist >= h_total) && (upper_dist >= h_total);
  double ha = h;
  unsigned char os = 0;
  if ((upper_dist >= lower_dist) && !central) {
    ha = fd_npmin(h, 0.5 * upper_dist / 1.0);
    os = 1;
  }
  if ((upper_dist < lower_dist) && !central) {
    ha = -fd_npmin(h, 0.5 * lower_dist / 1.0);
    os = 1;
  }
  const double min_dist = fd_npmin(upper_dist, lower_dist) / 1.0;
  if (!central && (fd_abs(ha) <= min_dist)) {
    ha = min_dist;
    os = 0;
  }
  *h_out = ha;
  *one_sided_out = os;
}

// One variable of _sparse_difference's perturbed points (:494-524, :541-544).  Returns whether
// dx was produced (the variable is a member of the group).
__host__ __device__ inline bool fd_perturb_one(int method, bool member, double x0, double h,
                                               unsigned char one_sided, double *x1, double *x2,
                                               double *dx) {
  const double h_vec = h * (member ? 1.0 : 0.0);
  if (method == FD_2POINT) {
    const double x = x0 + h_vec;
    *x1 = x;
    *dx = x - x0;
    return member;
  }
  if (method == FD_CS) {
    *x1 = h_vec;
    *dx = h_vec;
    return member;
  }
  double a = x0, b = x0;
  if (member && one_sided) {
    a = a + h_vec;
    b = b + 2.0 * h_vec;
    *dx = b - x0;
  } else if (member) {
    a = a - h_vec;
    b = b + h_vec;
    *dx = b - a;
  }
  *x1 = a;
  *x2 = b;
  return member;
}

// df[i] / dx[j] of one entry (:500, :537-540, :543, :555).
__host__ __device__ inline double fd_quotient(int method, unsigned char one_sided, double f0,
                                              double f1, double f2, double dx) {
  double df;
  if (method == FD_2POINT) df = f1 - f0;
  else if (method == FD_CS) df = f1;
  else if (one_sided) df = ((-3.0 * f0) + (4.0 * f1)) - f2;
  else df = f2 - f1;
  return df / dx;
}

constexpr double FD_INF = __builtin_huge_val();

__global__ void __launch_bounds__(IPX_BLOCK)
k_fd_steps(int64_t n, int method, double rel, const double *__restrict__ rel_vec,
           const double *__restrict__ x0, const double *__restrict__ lb,
           const double *__restrict__ ub, double *__restrict__ h,
           unsigned char *__restrict__ one_sided) {
  const int64_t stride = (int64_t)gridDim.x * IPX_BLOCK;
  for (int64_t j = (int64_t)blockIdx.x * IPX_BLOCK + threadIdx.x; j < n; j += stride) {
    double hj;
    unsigned char os;
    fd_step(method, rel_vec ? rel_vec[j] : rel, x0[j], lb ? lb[j] : -FD_INF, ub ? ub[j] : FD_INF,
            &hj, &os);
    h[j] = hj;
    one_sided[j] = os;
  }
}

__global__ void __launch_bounds__(IPX_BLOCK)
k_fd_perturb(int64_t n, int method, int g, const int32_t *__restrict__ groups,
             const double *__restrict__ x0, const double *__restrict__ h,
             const unsigned char *__restrict__ one_sided, double *__restrict__ x1,
             double *__restrict__ x2, double *__restrict__ dx) {
  const int64_t stride = (int64_t)gridDim.x * IPX_BLOCK;
  for (int64_t j = (int64_t)blockIdx.x * IPX_BLOCK + threadIdx.x; j < n; j += stride) {
    double a, b = 0.0, d = 0.0;
    const bool member = fd_perturb_one(method, groups[j] == g, x0[j], h[j],
                                       one_sided ? one_sided[j] : 0, &a, &b, &d);
    x1[j] = a;
    if (method == FD_3POINT) x2[j] = b;
    if (member) dx[j] = d;
  }
}

constexpr int TILE_NNZ = IPX_SPMV_TILE_NNZ;
constexpr int TILE_ROWS = IPX_SPMV_TILE_ROWS;

// One workgroup per SpMV row tile (a contiguous range [s, e) of stored entries, rows [r0, r1)):
// lane t takes entries s + t, s + t + 256, ... so col / val accesses are coalesced.  The row of an
// entry is found by bisection of the tile's slice of rowptr (in LDS; empty rows are skipped by
// taking the LAST row that starts at or before the entry).  All loads of one dependency level
// are issued for the lane's whole batch before the next level uses them.
template <int METHOD>
__global__ void __launch_bounds__(IPX_BLOCK)
k_fd_assemble(int64_t m, int64_t n, const int32_t *__restrict__ rowptr,
              const int32_t *__restrict__ colidx, const int32_t *__restrict__ tiles, int ntiles,
              const int32_t *__restrict__ groups, int g_lo, int g_hi,
              const double *__restrict__ f0, const double *__restrict__ F1,
              const double *__restrict__ F2, const double *__restrict__ dx,
              const unsigned char *__restrict__ one_sided, double *__restrict__ val) {
  __shared__ int rp[TILE_ROWS + 1];
  const int tile = ipx_xcd_item(blockIdx.x, ntiles);
  if (tile < 0) return;
  const int r0 = tiles[tile], r1 = tiles[tile + 1];
  const int s = tiles[ntiles + 1 + tile], e = tiles[ntiles + 2 + tile];
  const int nrows = r1 - r0;
  if (e <= s || nrows <= 0) return;
  const bool staged = nrows <= TILE_ROWS;          // (uniform over the workgroup)
  if (staged) {
    for (int i = threadIdx.x; i <= nrows; i += IPX_BLOCK) rp[i] = rowptr[r0 + i];
    __syncthreads();
  }
  const int ng = g_hi - g_lo;
  constexpr int U = TILE_NNZ / IPX_BLOCK;
  for (int base = s + (int)threadIdx.x; base < e; base += U * IPX_BLOCK) {
    int c[U], row[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = min(base + u * IPX_BLOCK, e - 1);
      int cu = colidx[k];
      c[u] = (cu >= 0 && (int64_t)cu < n) ? cu : 0;          // (a bad index reads column 0)
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = min(base + u * IPX_BLOCK, e - 1);
      int lo = 0, hi = nrows;                      // rowptr[r0 + lo] <= k < rowptr[r0 + hi]
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        const int v = staged ? rp[mid] : rowptr[r0 + mid];
        if (v <= k) lo = mid; else hi = mid;
      }
      row[u] = r0 + lo;
    }
    int gl[U];
    double d[U], a0[U];
    unsigned char os[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      gl[u] = groups[c[u]] - g_lo;
      d[u] = dx[c[u]];
      os[u] = (METHOD == FD_3POINT) ? one_sided[c[u]] : 0;
      a0[u] = (METHOD == FD_CS) ? 0.0 : f0[row[u]];
    }
    double a1[U], a2[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool mine = gl[u] >= 0 && gl[u] < ng;
      const int64_t at = mine ? (int64_t)gl[u] * m + row[u] : 0;
      a1[u] = F1[at];
      a2[u] = (METHOD == FD_3POINT) ? F2[at] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = base + u * IPX_BLOCK;
      if (k < e && gl[u] >= 0 && gl[u] < ng)
        val[k] = fd_quotient(METHOD, os[u], a0[u], a1[u], a2[u], d[u]);
    }
  }
}

// The symmetric assemble of a finite-difference HESSIAN (m = n, a structurally symmetric
// pattern): entry (i, j) gets 0.5 * (q_ij + q_ji), q_ij the quotient k_fd_assemble would write at
// (i, j) and q_ji the one it would write at (j, i) -- both read straight from the planes, so
// there is no second pass and no transposition table.  Same launch shape as k_fd_assemble (one
// workgroup per SpMV row tile, entries strided over the lanes, the row by bisection of the LDS
// copy of the tile's rowptr slice, the loads of one dependency level issued for the lane's batch
// before the next level uses them); an entry gathers twice as much, so a batch is 4 entries.
//
// Chunks of groups [g_lo, g_hi): a launch adds 0.5 * q_ij where g(j) is in range and 0.5 * q_ji
// where g(i) is.  Scaling by 0.5 is exact (barring underflow) and the two-term sum commutative,
// so 0.5 * q_ij + 0.5 * q_ji carries the bits of 0.5 * (q_ij + q_ji) whichever chunk brings
// which half: chunked results equal single-launch results bit for bit.  An entry is FRESH in
// the launch whose range holds min(g(i), g(j)) (chunks ascend): a fresh entry is written unless
// `accumulate`, any other is added to.  `slot` (NULL: k) places entry k in a value array on a
// larger pattern; a launch touches each slot once, so no atomics.
template <int METHOD>
__global__ void __launch_bounds__(IPX_BLOCK)
k_fd_assemble_sym(int64_t n, const int32_t *__restrict__ rowptr,
                  const int32_t *__restrict__ colidx, const int32_t *__restrict__ tiles,
                  int ntiles, const int32_t *__restrict__ groups, int g_lo, int g_hi,
                  const double *__restrict__ f0, const double *__restrict__ F1,
                  const double *__restrict__ F2, const double *__restrict__ dx,
                  const unsigned char *__restrict__ one_sided, const int32_t *__restrict__ slot,
                  int accumulate, double *__restrict__ val) {
  __shared__ int rp[TILE_ROWS + 1];
  const int tile = ipx_xcd_item(blockIdx.x, ntiles);
  if (tile < 0) return;
  const int r0 = tiles[tile], r1 = tiles[tile + 1];
  const int s = tiles[ntiles + 1 + tile], e = tiles[ntiles + 2 + tile];
  const int nrows = r1 - r0;
  if (e <= s || nrows <= 0) return;
  const bool staged = nrows <= TILE_ROWS;          // (uniform over the workgroup)
  if (staged) {
    for (int i = threadIdx.x; i <= nrows; i += IPX_BLOCK) rp[i] = rowptr[r0 + i];
    __syncthreads();
  }
  const int ng = g_hi - g_lo;
  constexpr int U = 4;
  for (int base = s + (int)threadIdx.x; base < e; base += U * IPX_BLOCK) {
    int c[U], row[U], at[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = min(base + u * IPX_BLOCK, e - 1);
      int cu = colidx[k];
      c[u] = (cu >= 0 && (int64_t)cu < n) ? cu : 0;          // (a bad index reads column 0)
      at[u] = slot ? slot[k] : k;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = min(base + u * IPX_BLOCK, e - 1);
      int lo = 0, hi = nrows;                      // rowptr[r0 + lo] <= k < rowptr[r0 + hi]
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        const int v = staged ? rp[mid] : rowptr[r0 + mid];
        if (v <= k) lo = mid; else hi = mid;
      }
      row[u] = r0 + lo;
    }
    int gc[U], gr[U];                              // group of the column / of the row, - g_lo
    double dc[U], dr[U], fr[U], fc[U];
    unsigned char oc[U], orow[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      gc[u] = groups[c[u]] - g_lo;
      gr[u] = groups[row[u]] - g_lo;
      dc[u] = dx[c[u]];
      dr[u] = dx[row[u]];
      oc[u] = (METHOD == FD_3POINT) ? one_sided[c[u]] : 0;
      orow[u] = (METHOD == FD_3POINT) ? one_sided[row[u]] : 0;
      fr[u] = (METHOD == FD_CS) ? 0.0 : f0[row[u]];
      fc[u] = (METHOD == FD_CS) ? 0.0 : f0[c[u]];
    }
    double a1[U], a2[U], b1[U], b2[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t pa = (gc[u] >= 0 && gc[u] < ng) ? (int64_t)gc[u] * n + row[u] : 0;
      const int64_t pb = (gr[u] >= 0 && gr[u] < ng) ? (int64_t)gr[u] * n + c[u] : 0;
      a1[u] = F1[pa];
      b1[u] = F1[pb];
      a2[u] = (METHOD == FD_3POINT) ? F2[pa] : 0.0;
      b2[u] = (METHOD == FD_3POINT) ? F2[pb] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = base + u * IPX_BLOCK;
      const bool ina = gc[u] >= 0 && gc[u] < ng, inb = gr[u] >= 0 && gr[u] < ng;
      if (k >= e || !(ina || inb)) continue;
      const double qa = 0.5 * fd_quotient(METHOD, oc[u], fr[u], a1[u], a2[u], dc[u]);
      const double qb = 0.5 * fd_quotient(METHOD, orow[u], fc[u], b1[u], b2[u], dr[u]);
      const double add = (ina && inb) ? qa + qb : (ina ? qa : qb);
      const bool fresh = gc[u] >= 0 && gr[u] >= 0;
      val[at[u]] = (fresh && !accumulate) ? add : val[at[u]] + add;
    }
  }
}

}  // namespace

extern "C" {

int ipx_fd_steps(int64_t n, int32_t method, double rel, const double *rel_vec, const double *x0,
                 const double *lb, const double *ub, double *h, unsigned char *one_sided,
                 void *stream) {
  if (n < 0 || method < FD_2POINT || method > FD_CS) return IPX_EINVAL;
  if (n == 0) return IPX_OK;
  if (!x0 || !h || !one_sided) return IPX_EINVAL;
  hipLaunchKernelGGL(k_fd_steps, dim3(ipx_grid_for(n, IPX_BLOCK, 2048)), dim3(IPX_BLOCK), 0,
                     (hipStream_t)stream, n, (int)method, rel, rel_vec, x0, lb, ub, h, one_sided);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

void ipx_fd_steps_host(int64_t n, int32_t method, double rel, const double *rel_vec,
                       const double *x0, const double *lb, const double *ub, double *h,
                       unsigned char *one_sided) {
  for (int64_t j = 0; j < n; ++j)
    fd_step(method, rel_vec ? rel_vec[j] : rel, x0[j], lb ? lb[j] : -FD_INF, ub ? ub[j] : FD_INF,
            &h[j], &one_sided[j]);
}

int ipx_fd_perturb(int64_t n, int32_t method, int32_t g, const int32_t *groups, const double *x0,
                   const double *h, const unsigned char *one_sided, double *x1, double *x2,
                   double *dx, void *stream) {
  if (n < 0 || method < FD_2POINT || method > FD_CS) return IPX_EINVAL;
  if (n == 0) return IPX_OK;
  if (!groups || !x0 || !h || !x1 || !dx || (method == FD_3POINT && (!x2 || !one_sided)))
    return IPX_EINVAL;
  hipLaunchKernelGGL(k_fd_perturb, dim3(ipx_grid_for(n, IPX_BLOCK, 2048)), dim3(IPX_BLOCK), 0,
                     (hipStream_t)stream, n, (int)method, (int)g, groups, x0, h, one_sided, x1, x2,
                     dx);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

void ipx_fd_perturb_host(int64_t n, int32_t method, int32_t g, const int32_t *groups,
                         const double *x0, const double *h, const unsigned char *one_sided,
                         double *x1, double *x2, double *dx) {
  for (int64_t j = 0; j < n; ++j) {
    double a, b = 0.0, d = 0.0;
    const bool member = fd_perturb_one(method, groups[j] == g, x0[j], h[j],
                                       one_sided ? one_sided[j] : 0, &a, &b, &d);
    x1[j] = a;
    if (method == FD_3POINT) x2[j] = b;
    if (member) dx[j] = d;
  }
}

int ipx_fd_assemble(int64_t m, int64_t n, const int32_t *rowptr, const int32_t *colidx,
                    const int32_t *tiles, int32_t ntiles, int32_t method, const int32_t *groups,
                    int32_t g_lo, int32_t g_hi, const double *f0, const double *F1,
                    const double *F2, const double *dx, const unsigned char *one_sided,
                    double *val, void *stream) {
  if (m < 0 || n < 0 || ntiles < 0 || method < FD_2POINT || method > FD_CS || g_lo < 0 ||
      g_hi < g_lo || m > INT32_MAX || n > INT32_MAX)
    return IPX_EINVAL;
  if (m == 0 || n == 0 || ntiles == 0 || g_hi == g_lo) return IPX_OK;
  if (!rowptr || !colidx || !tiles || !groups || !F1 || !dx || !val ||
      (method != FD_CS && !f0) || (method == FD_3POINT && (!F2 || !one_sided)))
    return IPX_EINVAL;
  const dim3 grid(ipx_xcd_grid(ntiles)), block(IPX_BLOCK);
  const hipStream_t st = (hipStream_t)stream;
  if (method == FD_2POINT)
    hipLaunchKernelGGL(k_fd_assemble<FD_2POINT>, grid, block, 0, st, m, n, rowptr, colidx, tiles,
                       (int)ntiles, groups, (int)g_lo, (int)g_hi, f0, F1, F2, dx, one_sided, val);
  else if (method == FD_3POINT)
    hipLaunchKernelGGL(k_fd_assemble<FD_3POINT>, grid, block, 0, st, m, n, rowptr, colidx, tiles,
                       (int)ntiles, groups, (int)g_lo, (int)g_hi, f0, F1, F2, dx, one_sided, val);
  else
    hipLaunchKernelGGL(k_fd_assemble<FD_CS>, grid, block, 0, st, m, n, rowptr, colidx, tiles,
                       (int)ntiles, groups, (int)g_lo, (int)g_hi, f0, F1, F2, dx, one_sided, val);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

void ipx_fd_assemble_host(int64_t m, int64_t n, const int32_t *rowptr, const int32_t *colidx,
                          int32_t method, const int32_t *groups, int32_t g_lo, int32_t g_hi,
                          const double *f0, const double *F1, const double *F2, const double *dx,
                          const unsigned char *one_sided, double *val) {
  for (int64_t i = 0; i < m; ++i)
    for (int32_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
      const int32_t c = colidx[k];
      if (c < 0 || c >= n) continue;
      const int32_t g = groups[c];
      if (g < g_lo || g >= g_hi) continue;
      const int64_t at = (int64_t)(g - g_lo) * m + i;
      val[k] = fd_quotient(method, (method == FD_3POINT) ? one_sided[c] : 0,
                           (method == FD_CS) ? 0.0 : f0[i], F1[at],
                           (method == FD_3POINT) ? F2[at] : 0.0, dx[c]);
    }
}

int ipx_fd_assemble_sym(int64_t n, const int32_t *rowptr, const int32_t *colidx,
                        const int32_t *tiles, int32_t ntiles, int32_t method,
                        const int32_t *groups, int32_t g_lo, int32_t g_hi, const double *f0,
                        const double *F1, const double *F2, const double *dx,
                        const unsigned char *one_sided, const int32_t *slot, int32_t accumulate,
                        double *val, void *stream) {
  if (n < 0 || ntiles < 0 || method < FD_2POINT || method > FD_CS || g_lo < 0 || g_hi < g_lo ||
      n > INT32_MAX)
    return IPX_EINVAL;
  if (n == 0 || ntiles == 0 || g_hi == g_lo) return IPX_OK;
  if (!rowptr || !colidx || !tiles || !groups || !F1 || !dx || !val ||
      (method != FD_CS && !f0) || (method == FD_3POINT && (!F2 || !one_sided)))
    return IPX_EINVAL;
  const dim3 grid(ipx_xcd_grid(ntiles)), block(IPX_BLOCK);
  const hipStream_t st = (hipStream_t)stream;
  if (method == FD_2POINT)
    hipLaunchKernelGGL(k_fd_assemble_sym<FD_2POINT>, grid, block, 0, st, n, rowptr, colidx, tiles,
                       (int)ntiles, groups, (int)g_lo, (int)g_hi, f0, F1, F2, dx, one_sided, slot,
                       (int)accumulate, val);
  else if (method == FD_3POINT)
    hipLaunchKernelGGL(k_fd_assemble_sym<FD_3POINT>, grid, block, 0, st, n, rowptr, colidx, tiles,
                       (int)ntiles, groups, (int)g_lo, (int)g_hi, f0, F1, F2, dx, one_sided, slot,
                       (int)accumulate, val);
  else
    hipLaunchKernelGGL(k_fd_assemble_sym<FD_CS>, grid, block, 0, st, n, rowptr, colidx, tiles,
                       (int)ntiles, groups, (int)g_lo, (int)g_hi, f0, F1, F2, dx, one_sided, slot,
                       (int)accumulate, val);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

void ipx_fd_assemble_sym_host(int64_t n, const int32_t *rowptr, const int32_t *colidx,
                              int32_t method, const int32_t *groups, int32_t g_lo, int32_t g_hi,
                              const double *f0, const double *F1, const double *F2,
                              const double *dx, const unsigned char *one_sided,
                              const int32_t *slot, int32_t accumulate, double *val) {
  for (int64_t i = 0; i < n; ++i)
    for (int32_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
      const int32_t c = colidx[k];
      if (c < 0 || c >= n) continue;
      const int32_t gc = groups[c] - g_lo, gr = groups[i] - g_lo, ng = g_hi - g_lo;
      const bool ina = gc >= 0 && gc < ng, inb = gr >= 0 && gr < ng;
      if (!(ina || inb)) continue;
      const bool three = method == FD_3POINT, cs = method == FD_CS;
      double qa = 0.0, qb = 0.0;
      if (ina) {
        const int64_t pa = (int64_t)gc * n + i;
        qa = 0.5 * fd_quotient(method, three ? one_sided[c] : 0, cs ? 0.0 : f0[i], F1[pa],
                               three ? F2[pa] : 0.0, dx[c]);
      }
      if (inb) {
        const int64_t pb = (int64_t)gr * n + c;
        qb = 0.5 * fd_quotient(method, three ? one_sided[i] : 0, cs ? 0.0 : f0[c], F1[pb],
                               three ? F2[pb] : 0.0, dx[i]);
      }
      const double add = (ina && inb) ? qa + qb : (ina ? qa : qb);
      const bool fresh = gc >= 0 && gr >= 0;
      const int64_t at = slot ? slot[k] : k;
      val[at] = (fresh && !accumulate) ? add : val[at] + add;
    }
}

}  // extern "C"
