// Sparse direct (A A')^-1 for any pattern: the numeric side of the nested-dissection solver
// (ipsolver/nested.py; the order and the symbolic factorization are host work,
// csrc/nested_order.hip).  A supernodal multifrontal Cholesky factorization, one elimination-tree
// level at a time.  include/ipx.h has the layout of a front and of the tables.
//   small fronts   (at most ND_SMALL_MAX rows) one workgroup per front, the front in LDS:
//                  assembly, the children's updates, the partial factorization -- one launch per
//                  level
//   large fronts   in global memory, own rows padded to whole 64-tiles: assembly and the
//                  children's updates batched over the level, then per front the tile-column
//                  steps of the dense Cholesky (csrc/dense.hip: fp64 matrix cores)
//   solves         one workgroup per front and one launch per level in either direction, the
//                  triangular solves in blocks of 64 columns: the diagonal block by one wave out
//                  of LDS, the rest of the column block as row (forward) or column (backward)
//                  sums of 64 terms
// Every sum has a fixed order and nothing is accumulated atomically.
#include "ipx_common.h"

namespace {

constexpr int NF = IPX_ND_FIELDS;
constexpr int ND_SMALL_MAX = 128;      // 128 x 129 doubles + the tables: 130.5 KB of LDS
constexpr int ND_SOLVE_MAX = 4096;     // rows of a front the solve kernels stage (32 KB)
constexpr int TB = 64;                 // column block of the solves = tile of the factorization

struct Front {
  int row0, s, b, ld, pad, c0, c1;
  int64_t bnd, off, work;
};

__host__ __device__ __forceinline__ Front front_of(const int64_t *sn, int j) {
  const int64_t *t = sn + (int64_t)j * NF;
  Front f;
  f.row0 = (int)t[0];
  f.s = (int)t[1];
  f.b = (int)t[2];
  f.bnd = t[3];
  f.off = t[4];
  f.ld = (int)t[5];
  f.pad = (int)t[6];
  f.c0 = (int)t[7];
  f.c1 = (int)t[8];
  f.work = t[9];
  return f;
}

// the row of A behind index i of a front
__device__ __forceinline__ int front_row(const ipx_nd_args &a, const Front &f, int i) {
  return i < f.s ? a.perm[f.row0 + i] : a.bnd_rows[f.bnd + (i - f.s)];
}

// entry (i, j) of A A': merge of the two sorted rows, the products added in storage order
__device__ __forceinline__ double aat_entry(const ipx_nd_args &a, int i, int j) {
  int p = a.A_rowptr[i], pe = a.A_rowptr[i + 1];
  int u = a.A_rowptr[j], ue = a.A_rowptr[j + 1];
  double sum = 0.0;
  while (p < pe && u < ue) {
    const int cp = a.A_colidx[p], cu = a.A_colidx[u];
    if (cp == cu) { sum += a.A_val[p] * a.A_val[u]; ++p; ++u; }
    else if (cp < cu) ++p;
    else ++u;
  }
  return sum;
}

// the update matrix a factored front leaves (row-major, leading dimension its ld)
__device__ __forceinline__ const double *update_of(const ipx_nd_args &a, const Front &c) {
  return a.fronts + c.off + (int64_t)(c.s + c.pad) * c.ld + (c.s + c.pad);
}

// ---------------------------------------------------------------- small fronts
// SKIP: the pivot-skipping factorization (rank-deficient A; ipsolver/nested.py
// PivotSkippingNestedSolver).  A pivot with |d| <= IPX_PIVOT_RTOL x its diagonal entry of S --
// row perm[k] of A depends on the rows eliminated before it, or is zero -- is skipped: its column
// of L is zero, its diagonal +inf, the trailing matrix takes no update, no bit is raised.  A
// pivot below -IPX_PIVOT_RTOL x the entry, or a NaN, stays bits 0 | 2.
template <bool SKIP>
__global__ void __launch_bounds__(IPX_BLOCK)
k_nd_factor_small(ipx_nd_args a, int64_t off, int assemble_only) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x;
  const Front f = front_of(a.sn, a.lists[off + blockIdx.x]);
  const int n = f.s + f.b, ldl = n | 1;
  double *F = lds;
  double *diag = F + (size_t)n * ldl;              // the diagonal of S, then of L
  int *rows = reinterpret_cast<int *>(diag + f.s);
  for (int i = tid; i < n; i += IPX_BLOCK) rows[i] = front_row(a, f, i);
  __syncthreads();
  for (int e = tid; e < f.s * n; e += IPX_BLOCK) {  // the own columns: entries of S
    const int c = e / n, r = e - c * n;
    if (r >= c) F[r * ldl + c] = aat_entry(a, rows[r], rows[c]);
  }
  for (int e = tid; e < f.b * f.b; e += IPX_BLOCK) {
    const int i = e / f.b, j = e - i * f.b;
    if (j <= i) F[(f.s + i) * ldl + f.s + j] = 0.0;
  }
  __syncthreads();
  for (int c = tid; c < f.s; c += IPX_BLOCK) diag[c] = F[c * ldl + c];
  __syncthreads();
  for (int ci = f.c0; ci < f.c1; ++ci) {            // the children, one after another
    const Front c = front_of(a.sn, a.child_idx[ci]);
    const int32_t *cm = a.cmap + c.bnd;
    const double *U = update_of(a, c);
    for (int e = tid; e < c.b * c.b; e += IPX_BLOCK) {
      const int i = e / c.b, j = e - i * c.b;
      if (j <= i) F[cm[i] * ldl + cm[j]] += U[(int64_t)i * c.ld + j];
    }
    __syncthreads();
  }
  int bits = 0;
  const int steps = assemble_only ? 0 : f.s;
  for (int k = 0; k < steps; ++k) {
    __syncthreads();
    const double d = F[k * ldl + k];
    // (SKIP: every thread reads diag[k] = S_kk here, so thread 0 stores the new diagonal only
    // behind the barrier)
    const bool skip = SKIP && fabs(d) <= IPX_PIVOT_RTOL * diag[k];
    const double lkk = skip ? __builtin_huge_val() : sqrt(d > 0.0 ? d : 1.0);
    for (int i = k + 1 + tid; i < n; i += IPX_BLOCK) {
      if (skip) F[i * ldl + k] = 0.0;
      else F[i * ldl + k] /= lkk;
    }
    if (tid == 0) {
      // bit 0: the pivot lost 43 bits against its diagonal entry of S (the factorization goes
      // on); bit 2: it is not positive (no factorization)
      if (!skip && !(d > IPX_PIVOT_RTOL * diag[k])) bits |= (d > 0.0) ? 1 : 5;
      if (!SKIP) diag[k] = lkk;
    }
    __syncthreads();
    if (SKIP && tid == 0) diag[k] = lkk;
    const int rem = n - k - 1;
    for (int e = tid; e < rem * rem; e += IPX_BLOCK) {
      const int i = e / rem, j = e - i * rem;
      if (j <= i) F[(k + 1 + i) * ldl + k + 1 + j] -= F[(k + 1 + i) * ldl + k] * F[(k + 1 + j) * ldl + k];
    }
  }
  __syncthreads();
  double *G = a.fronts + f.off;
  for (int e = tid; e < n * n; e += IPX_BLOCK) {
    const int r = e / n, c = e - r * n;
    // (above the diagonal: the factor's columns once more as rows, for the forward solve)
    G[e] = c > r ? (r < steps ? F[c * ldl + r] : 0.0) : (c == r && r < steps) ? diag[r] : F[r * ldl + c];
  }
  if (tid == 0 && bits) atomicOr(a.flag, bits);
}

// ---------------------------------------------------------------- large fronts
// index of a front behind storage row r: -1 for a unit-diagonal padding row, -2 for a zero row
__device__ __forceinline__ int front_index(const Front &f, int r) {
  if (r < f.s) return r;
  if (r < f.s + f.pad) return -1;
  return r - f.pad < f.s + f.b ? r - f.pad : -2;
}

__global__ void __launch_bounds__(IPX_BLOCK) k_nd_assemble_large(ipx_nd_args a, int64_t off) {
  const Front f = front_of(a.sn, a.lists[off + blockIdx.y]);
  double *G = a.fronts + f.off;
  double *work = a.work + f.work;
  const int64_t tot = (int64_t)f.ld * f.ld;
  for (int64_t e = (int64_t)blockIdx.x * IPX_BLOCK + threadIdx.x; e < tot;
       e += (int64_t)gridDim.x * IPX_BLOCK) {
    const int r = (int)(e / f.ld), c = (int)(e - (int64_t)r * f.ld);
    const int fr = front_index(f, r), fc = front_index(f, c);
    double v = 0.0;
    if (c <= r) {
      if (fr == -1) v = (r == c) ? 1.0 : 0.0;
      else if (fr >= 0 && fc >= 0 && fc < f.s) v = aat_entry(a, front_row(a, f, fr), front_row(a, f, fc));
    }
    G[e] = v;
    if (r == c) work[r] = (fr >= 0 && fr < f.s) ? v : 1.0;
    if (e == 0) work[f.ld] = 1.0;
  }
}

// the update of child number q of every front of the list
__global__ void __launch_bounds__(IPX_BLOCK) k_nd_extend_add(ipx_nd_args a, int64_t off, int q) {
  const Front f = front_of(a.sn, a.lists[off + blockIdx.y]);
  if (f.c0 + q >= f.c1) return;
  const Front c = front_of(a.sn, a.child_idx[f.c0 + q]);
  const int32_t *cm = a.cmap + c.bnd;
  const double *U = update_of(a, c);
  double *G = a.fronts + f.off;
  const int64_t tot = (int64_t)c.b * c.b;
  for (int64_t e = (int64_t)blockIdx.x * IPX_BLOCK + threadIdx.x; e < tot;
       e += (int64_t)gridDim.x * IPX_BLOCK) {
    const int i = (int)(e / c.b), j = (int)(e - (int64_t)i * c.b);
    if (j > i) continue;
    const int pi = cm[i], pj = cm[j];
    const int r = pi < f.s ? pi : pi + f.pad, cc = pj < f.s ? pj : pj + f.pad;
    G[(int64_t)r * f.ld + cc] += U[(int64_t)i * c.ld + j];
  }
}

// L' into the rows of the factor's columns, above the diagonal (what the forward solve reads):
// 32 x 32 tiles through LDS, both sides coalesced
__global__ void __launch_bounds__(IPX_BLOCK) k_nd_mirror(ipx_nd_args a, int64_t off) {
  __shared__ double tile[32][33];
  const Front f = front_of(a.sn, a.lists[off + blockIdx.y]);
  double *G = a.fronts + f.off;
  const int nt = f.ld / 32, kt = (f.s + f.pad) / 32;          // tiles per side, factor tile columns
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int t = blockIdx.x; t < kt * nt; t += gridDim.x) {
    const int tc = t / nt, tr = t - tc * nt;                  // tile (tr, tc) of L, tr >= tc
    if (tr < tc) continue;
    __syncthreads();
    for (int y = ty; y < 32; y += 8) tile[y][tx] = G[(int64_t)(tr * 32 + y) * f.ld + tc * 32 + tx];
    __syncthreads();
    for (int y = ty; y < 32; y += 8) {
      const int r = tc * 32 + y, cc = tr * 32 + tx;           // entry (r, cc) = L[cc][r]
      if (cc > r) G[(int64_t)r * f.ld + cc] = tile[tx][y];
    }
  }
}

// ---------------------------------------------------------------- solves
__device__ __forceinline__ void stage_block(const double *G, int ld, int kb, int nb, double *T) {
  for (int e = threadIdx.x; e < nb * TB; e += IPX_BLOCK) {
    const int r = e >> 6, c = e & (TB - 1);
    if (c < nb) T[r * (TB + 1) + c] = G[(int64_t)(kb + r) * ld + kb + c];
  }
}

__global__ void __launch_bounds__(IPX_BLOCK)
k_nd_forward(ipx_nd_args a, int64_t off, const double *__restrict__ w, int xcap) {
  extern __shared__ double lds[];
  double *x = lds, *T = lds + xcap;
  const int tid = threadIdx.x;
  const Front f = front_of(a.sn, a.lists[off + blockIdx.x]);
  const int n = f.s + f.b;
  const double *G = a.fronts + f.off;
  for (int i = tid; i < n; i += IPX_BLOCK) x[i] = i < f.s ? w[a.perm[f.row0 + i]] : 0.0;
  __syncthreads();
  for (int ci = f.c0; ci < f.c1; ++ci) {
    const Front c = front_of(a.sn, a.child_idx[ci]);
    const int32_t *cm = a.cmap + c.bnd;
    for (int i = tid; i < c.b; i += IPX_BLOCK) x[cm[i]] += a.upd[c.bnd + i];
    __syncthreads();
  }
  for (int kb = 0; kb < f.s; kb += TB) {
    const int nb = min(TB, f.s - kb);
    stage_block(G, f.ld, kb, nb, T);
    __syncthreads();
    if (tid < IPX_WAVE) {
      double xv = tid < nb ? x[kb + tid] : 0.0;
      for (int k = 0; k < nb; ++k) {
        // A DIVISION, not a multiply by a reciprocal formed elsewhere: a skipped pivot
        // (pivot-skipping factorization) is stored as +inf over a zero column, and x / inf = 0
        // for every finite x is what makes this solve the one with the kept rows only.
        const double xk = __shfl(xv, k, IPX_WAVE) / T[k * (TB + 1) + k];
        if (tid == k) xv = xk;
        else if (tid > k && tid < nb) xv -= T[tid * (TB + 1) + k] * xk;
      }
      if (tid < nb) x[kb + tid] = xv;
    }
    __syncthreads();
    for (int i = kb + nb + tid; i < n; i += IPX_BLOCK) {     // every row below the block: its
      // entries L[i][kb + k] out of the mirror, a row of the store per k
      const double *col = G + (int64_t)kb * f.ld + (i < f.s ? i : i + f.pad);
      double acc = 0.0;
#pragma unroll 8
      for (int k = 0; k < nb; ++k) acc += col[(int64_t)k * f.ld] * x[kb + k];
      x[i] -= acc;
    }
    __syncthreads();
  }
  for (int i = tid; i < f.s; i += IPX_BLOCK) a.y[f.row0 + i] = x[i];
  for (int i = tid; i < f.b; i += IPX_BLOCK) a.upd[f.bnd + i] = x[f.s + i];
}

__global__ void __launch_bounds__(IPX_BLOCK)
k_nd_backward(ipx_nd_args a, int64_t off, double *__restrict__ xg, int xcap) {
  extern __shared__ double lds[];
  double *x = lds, *T = lds + xcap;
  const int tid = threadIdx.x;
  const Front f = front_of(a.sn, a.lists[off + blockIdx.x]);
  const int n = f.s + f.b;
  const double *G = a.fronts + f.off;
  for (int i = tid; i < n; i += IPX_BLOCK)
    x[i] = i < f.s ? a.y[f.row0 + i] : xg[a.bnd_rows[f.bnd + (i - f.s)]];
  __syncthreads();
  for (int k = tid; k < f.s; k += IPX_BLOCK) {               // y - L21' x2, a column per lane
    const double *col = G + (int64_t)(f.s + f.pad) * f.ld + k;
    double acc = 0.0;
#pragma unroll 8
    for (int i = 0; i < f.b; ++i) acc += col[(int64_t)i * f.ld] * x[f.s + i];
    x[k] -= acc;
  }
  __syncthreads();
  for (int kb = ((f.s - 1) / TB) * TB; kb >= 0; kb -= TB) {
    const int nb = min(TB, f.s - kb);
    stage_block(G, f.ld, kb, nb, T);
    __syncthreads();
    if (tid < IPX_WAVE) {
      double xv = tid < nb ? x[kb + tid] : 0.0;
      for (int k = nb - 1; k >= 0; --k) {
        // (a division on purpose, as in k_nd_forward: x / inf = 0 for a skipped pivot, whose
        // row's entries in the earlier columns are then multiplied by that zero)
        const double xk = __shfl(xv, k, IPX_WAVE) / T[k * (TB + 1) + k];
        if (tid == k) xv = xk;
        else if (tid < k) xv -= T[k * (TB + 1) + tid] * xk;
      }
      if (tid < nb) x[kb + tid] = xv;
    }
    __syncthreads();
    for (int j = tid; j < kb; j += IPX_BLOCK) {              // the columns before the block
      const double *col = G + (int64_t)kb * f.ld + j;
      double acc = 0.0;
#pragma unroll 8
      for (int k = 0; k < nb; ++k) acc += col[(int64_t)k * f.ld] * x[kb + k];
      x[j] -= acc;
    }
    __syncthreads();
  }
  for (int i = tid; i < f.s; i += IPX_BLOCK) xg[a.perm[f.row0 + i]] = x[i];
}

// ---------------------------------------------------------------- pivot-skipping: the dropped rows
// mark[row] = 1 where the stored diagonal of the row's own position is +inf, else 0: a workgroup
// per front over its own rows (every row of A is an own row of exactly one front)
__global__ void __launch_bounds__(IPX_BLOCK) k_nd_skipped(ipx_nd_args a, int32_t *mark) {
  const Front f = front_of(a.sn, (int)blockIdx.x);
  const double *G = a.fronts + f.off;
  for (int i = threadIdx.x; i < f.s; i += IPX_BLOCK)
    mark[a.perm[f.row0 + i]] = G[(int64_t)i * f.ld + i] == __builtin_huge_val() ? 1 : 0;
}

// t[i] = 0 for a dropped row, else b[i] + sum_j Y[i + m j] b[d_rows[j]] (j ascending)
__global__ void __launch_bounds__(IPX_BLOCK)
k_nd_dropped_fold(int64_t m, int q, const double *__restrict__ Y, const int32_t *__restrict__ d_rows,
                  const int32_t *__restrict__ mark, const double *__restrict__ b,
                  double *__restrict__ t) {
  __shared__ double bd[32];
  if ((int)threadIdx.x < q) bd[threadIdx.x] = b[d_rows[threadIdx.x]];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * IPX_BLOCK + threadIdx.x;
  if (i >= m) return;
  double v = 0.0;
  if (!mark[i]) {
    v = b[i];
    for (int j = 0; j < q; ++j) v += Y[i + m * j] * bd[j];
  }
  t[i] = v;
}

// out[i] = u[i] for a kept row; out[d_rows[j]] = sum_g part[g * q + j] (g ascending): the last
// q threads of the launch, a dropped row each
__global__ void __launch_bounds__(IPX_BLOCK)
k_nd_dropped_fill(int64_t m, int q, int groups, const double *__restrict__ part,
                  const int32_t *__restrict__ d_rows, const int32_t *__restrict__ mark,
                  const double *__restrict__ u, double *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * IPX_BLOCK + threadIdx.x;
  if (i < m) {
    if (!mark[i]) out[i] = u[i];
  } else if (i < m + q) {
    const int j = (int)(i - m);
    double sum = 0.0;
    for (int g = 0; g < groups; ++g) sum += part[(int64_t)g * q + j];
    out[d_rows[j]] = sum;
  }
}

int bad_args(const ipx_nd_args *a, int64_t off, int64_t cnt) {
  return !a || off < 0 || cnt < 0 || off + cnt > a->nsuper || !a->sn || !a->perm || !a->lists ||
         !a->fronts || !a->flag || !a->y;
}

template <class K>
int raise_lds(K kernel, size_t bytes) {
  if (bytes <= 65536) return IPX_OK;                 // (within the limit every kernel has)
  const hipError_t e = hipFuncSetAttribute((const void *)kernel,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) {
    ipx_note_error(e, __FILE__, __LINE__);
    return IPX_ELAUNCH;
  }
  return IPX_OK;
}

size_t solve_lds(int xcap) { return sizeof(double) * ((size_t)xcap + TB * (TB + 1)); }

// one level upwards
int nd_forward(const ipx_nd_args *a, int64_t off, int64_t cnt, int32_t fmax, const double *w,
               void *stream) {
  if (bad_args(a, off, cnt) || fmax < 1 || fmax > ND_SOLVE_MAX || !w || !a->upd) return IPX_EINVAL;
  if (cnt == 0) return IPX_OK;
  if (raise_lds(k_nd_forward, solve_lds(fmax)) != IPX_OK) return IPX_ELAUNCH;
  hipLaunchKernelGGL(k_nd_forward, dim3((unsigned)cnt), dim3(IPX_BLOCK), solve_lds(fmax),
                     (hipStream_t)stream, *a, off, w, (int)fmax);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

// one level downwards
int nd_backward(const ipx_nd_args *a, int64_t off, int64_t cnt, int32_t fmax, double *x,
                void *stream) {
  if (bad_args(a, off, cnt) || fmax < 1 || fmax > ND_SOLVE_MAX || !x) return IPX_EINVAL;
  if (cnt == 0) return IPX_OK;
  if (raise_lds(k_nd_backward, solve_lds(fmax)) != IPX_OK) return IPX_ELAUNCH;
  hipLaunchKernelGGL(k_nd_backward, dim3((unsigned)cnt), dim3(IPX_BLOCK), solve_lds(fmax),
                     (hipStream_t)stream, *a, off, x, (int)fmax);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

// small fronts of one level with the given kernel (k_nd_factor_small<false> or <true>)
int nd_factor_small_launch(void (*kernel)(ipx_nd_args, int64_t, int), const ipx_nd_args *a,
                           int64_t off, int64_t cnt, int32_t fmax, int32_t assemble_only,
                           void *stream) {
  if (bad_args(a, off, cnt) || fmax < 1 || fmax > ND_SMALL_MAX || !a->A_rowptr || !a->A_val)
    return IPX_EINVAL;
  if (cnt == 0) return IPX_OK;
  const size_t lds = sizeof(double) * ((size_t)fmax * (fmax | 1) + fmax) + sizeof(int) * fmax;
  if (raise_lds(kernel, lds) != IPX_OK) return IPX_ELAUNCH;
  hipLaunchKernelGGL(kernel, dim3((unsigned)cnt), dim3(IPX_BLOCK), lds, (hipStream_t)stream, *a,
                     off, (int)assemble_only);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

// large fronts of one level; skip: the pivot-skipping diagonal-tile kernel
int nd_factor_large(const ipx_nd_args *a, const int64_t *sn_host, const int32_t *lists_host,
                    int64_t off, int64_t cnt, int32_t assemble_only, int skip, void *stream) {
  if (bad_args(a, off, cnt) || !sn_host || !lists_host || !a->work || !a->A_rowptr || !a->A_val ||
      cnt > 65535)
    return IPX_EINVAL;
  if (cnt == 0) return IPX_OK;
  hipStream_t st = (hipStream_t)stream;
  int ldmax = 0, qmax = 0;
  for (int64_t t = 0; t < cnt; ++t) {
    const Front f = front_of(sn_host, lists_host[off + t]);
    if (f.ld < TB || f.ld % TB || (f.s + f.pad) % TB || f.s + f.pad + f.b > f.ld) return IPX_EINVAL;
    ldmax = f.ld > ldmax ? f.ld : ldmax;
    qmax = f.c1 - f.c0 > qmax ? f.c1 - f.c0 : qmax;
  }
  const dim3 grid((unsigned)ipx_grid_for((int64_t)ldmax * ldmax, IPX_BLOCK, 2048), (unsigned)cnt);
  hipLaunchKernelGGL(k_nd_assemble_large, grid, dim3(IPX_BLOCK), 0, st, *a, off);
  IPX_CHECK_LAUNCH();
  for (int q = 0; q < qmax; ++q) {
    hipLaunchKernelGGL(k_nd_extend_add, grid, dim3(IPX_BLOCK), 0, st, *a, off, q);
    IPX_CHECK_LAUNCH();
  }
  for (int64_t t = 0; t < cnt && !assemble_only; ++t) {
    const Front f = front_of(sn_host, lists_host[off + t]);
    const int rc = (skip ? ipx_chol_factor_steps_skip : ipx_chol_factor_steps)(
        f.ld, a->fronts + f.off, (f.s + f.pad) / TB, reinterpret_cast<int *>(a->flag),
        a->work + f.work, stream);
    if (rc != IPX_OK) return rc;
  }
  if (!assemble_only) {
    hipLaunchKernelGGL(k_nd_mirror, dim3(256, (unsigned)cnt), dim3(IPX_BLOCK), 0, st, *a, off);
    IPX_CHECK_LAUNCH();
  }
  return IPX_OK;
}

}  // namespace

extern "C" {

int ipx_nd_small_max(void) { return ND_SMALL_MAX; }

int ipx_nd_factor_small(const ipx_nd_args *a, int64_t off, int64_t cnt, int32_t fmax,
                        int32_t assemble_only, void *stream) {
  return nd_factor_small_launch(k_nd_factor_small<false>, a, off, cnt, fmax, assemble_only, stream);
}

int ipx_nd_factor_small_skip(const ipx_nd_args *a, int64_t off, int64_t cnt, int32_t fmax,
                             int32_t assemble_only, void *stream) {
  return nd_factor_small_launch(k_nd_factor_small<true>, a, off, cnt, fmax, assemble_only, stream);
}

int ipx_nd_factor_large(const ipx_nd_args *a, const int64_t *sn_host, const int32_t *lists_host,
                        int64_t off, int64_t cnt, int32_t assemble_only, void *stream) {
  return nd_factor_large(a, sn_host, lists_host, off, cnt, assemble_only, 0, stream);
}

int ipx_nd_factor_large_skip(const ipx_nd_args *a, const int64_t *sn_host,
                             const int32_t *lists_host, int64_t off, int64_t cnt,
                             int32_t assemble_only, void *stream) {
  return nd_factor_large(a, sn_host, lists_host, off, cnt, assemble_only, 1, stream);
}

int ipx_nd_skipped(const ipx_nd_args *a, int32_t *mark, void *stream) {
  if (bad_args(a, 0, 0) || !mark) return IPX_EINVAL;
  if (a->nsuper == 0) return IPX_OK;
  hipLaunchKernelGGL(k_nd_skipped, dim3((unsigned)a->nsuper), dim3(IPX_BLOCK), 0,
                     (hipStream_t)stream, *a, mark);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

int ipx_nd_dropped_fold(int64_t m, int32_t q, const double *Y, const int32_t *d_rows,
                        const int32_t *mark, const double *b, double *t, void *stream) {
  if (m < 1 || q < 0 || q > 32 || !mark || !b || !t || (q > 0 && (!Y || !d_rows)))
    return IPX_EINVAL;
  hipLaunchKernelGGL(k_nd_dropped_fold, dim3((unsigned)((m + IPX_BLOCK - 1) / IPX_BLOCK)),
                     dim3(IPX_BLOCK), 0, (hipStream_t)stream, m, (int)q, Y, d_rows, mark, b, t);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

int ipx_nd_dropped_fill(int64_t m, int32_t q, const double *part, const int32_t *d_rows,
                        const int32_t *mark, const double *u, double *out, void *stream) {
  if (m < 1 || q < 1 || q > 32 || !part || !d_rows || !mark || !u || !out) return IPX_EINVAL;
  const int groups = ipx_border_groups(m);
  hipLaunchKernelGGL(k_nd_dropped_fill, dim3((unsigned)((m + q + IPX_BLOCK - 1) / IPX_BLOCK)),
                     dim3(IPX_BLOCK), 0, (hipStream_t)stream, m, (int)q, groups, part, d_rows, mark,
                     u, out);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

// A whole solve: the levels upwards, then downwards.  levels_host: per level (offset into the
// lists, number of fronts, the largest front).
int ipx_nd_solve(const ipx_nd_args *a, int32_t nlevels, const int64_t *levels_host, const double *w,
                 double *x, void *stream) {
  if (nlevels < 0 || (nlevels > 0 && !levels_host)) return IPX_EINVAL;
  for (int l = 0; l < nlevels; ++l) {
    const int64_t *t = levels_host + 3 * l;
    const int rc = nd_forward(a, t[0], t[1], (int32_t)t[2], w, stream);
    if (rc != IPX_OK) return rc;
  }
  for (int l = nlevels - 1; l >= 0; --l) {
    const int64_t *t = levels_host + 3 * l;
    const int rc = nd_backward(a, t[0], t[1], (int32_t)t[2], x, stream);
    if (rc != IPX_OK) return rc;
  }
  return IPX_OK;
}

}  // extern "C"
