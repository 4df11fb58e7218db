// Bordered direct (A A')^-1: a few dense columns on top of a banded / block-tridiagonal solve.
//
// A = [B | C], C the p <= 32 columns that reach (nearly) every row: S = A A' = S_B + C C' with
// S_B = B B' a matrix the direct solvers factor.  Woodbury:
//     S^-1 w = u - Y K^-1 Y' w,   u = S_B^-1 w,   Y = S_B^-1 C,   K = I_p + C' Y   (K >= I).
// The inner solves (u, and the p columns of Y once per factorization) are the caller's; this
// file holds the O(m p) and O(m p^2) rest.  C and Y are column-major m x p, K and its Cholesky
// factor row-major p x p; Python owns every buffer, nothing is allocated and no handle is kept.
//
// Rows are dealt in chunks of BD_ROWS = 256 (a row per lane); a launch has
// G = min(ceil(m / 256), 512) workgroups, group g takes chunks g, g + G, ...  Every sum has a
// fixed order (per lane over its chunks, DPP wave sum, the waves and then the groups in
// ascending order; no atomics): the same values give the same bits, and since every operation is
// a sum of products, a correctly rounded division or a square root of K -- which does not change
// when A is scaled by a power of two -- a scaled A gives the scaled result bit for bit.
//
//   ipx_border_scatter   C from A's values (zero fill, then one entry per index pair)
//   ipx_border_gram      stage 1: per group the p x p partial of C' Y, the chunk staged through
//                        LDS in tiles of 64 rows; stage 2 (one workgroup): K = I + the partials
//                        in group order, its Cholesky factor in LDS, flag and trace(K)
//   ipx_border_tdot      per group the p partial sums of t = Y' w
//   ipx_border_apply     every workgroup folds the partials of t in the same order, solves
//                        L L' z = t in LDS (one wave, the unknowns in its lanes), and writes
//                        v = u - Y z for its rows
//
// Pivot signals of K (as for every factorization here): bit 0 -- a pivot below 2^-43 of its
// diagonal entry; bits 0 and 2 -- a pivot <= 0 (1 takes its place: nothing faults).
#include "ipx_common.h"

namespace {

constexpr int BD_PMAX = 32;
constexpr int BD_ROWS = IPX_BLOCK;         // rows of a chunk: one per lane
constexpr int BD_GROUP_CAP = 512;          // partials per quantity, at most
constexpr int BD_APPLY_CAP = 1024;         // workgroups of the apply kernel, at most
constexpr int BD_TILE = 64;                // rows of a Gram tile in LDS
constexpr int BD_PAD = BD_PMAX + 1;        // LDS row stride (doubles): rows on distinct banks
constexpr int BD_FOLD = IPX_BLOCK / BD_PMAX;   // 8 strided partial sums per entry of t

__host__ __device__ inline int64_t bd_chunks(int64_t m) { return (m + BD_ROWS - 1) / BD_ROWS; }
inline int bd_groups(int64_t m) {
  const int64_t c = bd_chunks(m);
  return (int)(c < BD_GROUP_CAP ? c : BD_GROUP_CAP);
}

__global__ void __launch_bounds__(IPX_BLOCK) k_bd_fill(int64_t n, double *__restrict__ C) {
  const int64_t i = (int64_t)blockIdx.x * IPX_BLOCK + threadIdx.x;
  if (i < n) C[i] = 0.0;
}

__global__ void __launch_bounds__(IPX_BLOCK)
k_bd_scatter(int64_t nnz, const double *__restrict__ val, const int32_t *__restrict__ src,
             const int64_t *__restrict__ dst, double *__restrict__ C) {
  const int64_t i = (int64_t)blockIdx.x * IPX_BLOCK + threadIdx.x;
  if (i < nnz) C[dst[i]] = val[src[i]];
}

// part[g][a][b] = sum over the rows of group g of C[r, a] Y[r, b]
__global__ void __launch_bounds__(IPX_BLOCK)
k_bd_gram_partial(int64_t m, int p, const double *__restrict__ C, const double *__restrict__ Y,
                  double *__restrict__ part) {
  __shared__ double Cs[BD_TILE * BD_PAD], Ys[BD_TILE * BD_PAD];
  const int tid = threadIdx.x, pp = p * p;
  constexpr int NQ = BD_PMAX * BD_PMAX / IPX_BLOCK;           // entries per lane: 4
  double acc[NQ];
  int ea[NQ], eb[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int e = tid + q * IPX_BLOCK;
    acc[q] = 0.0;
    ea[q] = e < pp ? e / p : 0;
    eb[q] = e < pp ? e % p : 0;
  }
  const int64_t chunks = bd_chunks(m);
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    for (int t = 0; t < BD_ROWS / BD_TILE; ++t) {
      const int64_t r0 = c * BD_ROWS + (int64_t)t * BD_TILE;
      if (r0 >= m) break;                                     // (uniform in the workgroup)
      __syncthreads();
      for (int idx = tid; idx < BD_TILE * p; idx += IPX_BLOCK) {
        const int j = idx / BD_TILE, rl = idx % BD_TILE;
        const int64_t r = r0 + rl;
        Cs[rl * BD_PAD + j] = r < m ? C[r + m * j] : 0.0;
        Ys[rl * BD_PAD + j] = r < m ? Y[r + m * j] : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        if (tid + q * IPX_BLOCK < pp) {
          double s = acc[q];
#pragma unroll 8
          for (int rl = 0; rl < BD_TILE; ++rl)
            s = __builtin_fma(Cs[rl * BD_PAD + ea[q]], Ys[rl * BD_PAD + eb[q]], s);
          acc[q] = s;
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int e = tid + q * IPX_BLOCK;
    if (e < pp) part[(int64_t)blockIdx.x * pp + e] = acc[q];
  }
}

// K = I + sum_g part[g] (ascending g), L = chol(K) (lower, row-major; zeros above the diagonal),
// info[0] = pivot bits, info[1] = trace(K).  One workgroup.
__global__ void __launch_bounds__(IPX_BLOCK)
k_bd_chol(int p, int G, const double *__restrict__ part, double *__restrict__ K,
          double *__restrict__ L, double *__restrict__ info) {
  __shared__ double T[BD_PMAX * BD_PAD], colv[BD_PMAX], d0[BD_PMAX];
  const int tid = threadIdx.x, pp = p * p;
  for (int e = tid; e < pp; e += IPX_BLOCK) {
    double s = 0.0;
#pragma unroll 8
    for (int g = 0; g < G; ++g) s += part[(int64_t)g * pp + e];
    const int a = e / p, b = e % p;
    const double k = a == b ? 1.0 + s : s;
    K[e] = k;
    T[a * BD_PAD + b] = k;
    if (a == b) d0[a] = k;
  }
  __syncthreads();
  int bits = 0;
  if (tid == 0) {
    double tr = 0.0;
    for (int j = 0; j < p; ++j) tr += d0[j];
    info[1] = tr;
  }
  // right-looking Cholesky on the lower triangle, a column per trip (as csrc/blocktri.hip)
  for (int j = 0; j < p; ++j) {
    const double d = T[j * BD_PAD + j];
    if (tid == 0 && !(d > IPX_PIVOT_RTOL * d0[j])) bits |= (d > 0.0) ? 1 : 5;
    const double l = sqrt(d > 0.0 ? d : 1.0);
    if (tid >= j && tid < p) colv[tid] = tid == j ? l : T[tid * BD_PAD + j] / l;
    __syncthreads();
    const int rem = p - j - 1;
    for (int e = tid; e < rem * rem; e += IPX_BLOCK) {
      const int i = j + 1 + e / rem, c = j + 1 + e % rem;
      if (c <= i) T[i * BD_PAD + c] = __builtin_fma(-colv[i], colv[c], T[i * BD_PAD + c]);
    }
    if (tid >= j && tid < p) T[tid * BD_PAD + j] = colv[tid];
    __syncthreads();
  }
  for (int e = tid; e < pp; e += IPX_BLOCK) {
    const int r = e / p, c = e % p;
    L[e] = c <= r ? T[r * BD_PAD + c] : 0.0;
  }
  if (tid == 0) info[0] = (double)bits;
}

// part[g][j] = sum over the rows of group g of Y[r, j] w[r]
__global__ void __launch_bounds__(IPX_BLOCK)
k_bd_tdot(int64_t m, int p, const double *__restrict__ Y, const double *__restrict__ w,
          double *__restrict__ part) {
  __shared__ double red[(IPX_BLOCK / IPX_WAVE) * BD_PMAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double acc[BD_PMAX];
#pragma unroll
  for (int j = 0; j < BD_PMAX; ++j) acc[j] = 0.0;
  const int64_t chunks = bd_chunks(m);
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const int64_t r = c * BD_ROWS + tid;
    if (r < m) {
      const double wr = w[r];
#pragma unroll
      for (int j = 0; j < BD_PMAX; ++j)
        if (j < p) acc[j] = __builtin_fma(Y[r + m * j], wr, acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < BD_PMAX; ++j) {
    if (j < p) {                                              // (uniform: all lanes active)
      const double s = ipx_wave_sum(acc[j]);
      if (lane == 0) red[wave * BD_PMAX + j] = s;
    }
  }
  __syncthreads();
  if (tid < p)
    part[(int64_t)blockIdx.x * p + tid] =
        ((red[tid] + red[BD_PMAX + tid]) + red[2 * BD_PMAX + tid]) + red[3 * BD_PMAX + tid];
}

// t = the partials folded, z = (L L')^-1 t, v[r] = u[r] - sum_j Y[r, j] z[j] (j ascending)
__global__ void __launch_bounds__(IPX_BLOCK)
k_bd_apply(int64_t m, int p, int G, const double *__restrict__ Y, const double *__restrict__ L,
           const double *__restrict__ part, const double *u, double *v) {
  __shared__ double Ls[BD_PMAX * BD_PAD], fold[BD_FOLD * BD_PMAX], z[BD_PMAX];
  const int tid = threadIdx.x;
  for (int e = tid; e < p * p; e += IPX_BLOCK) Ls[(e / p) * BD_PAD + e % p] = L[e];
  {
    // entry j of t: 8 lanes take the groups g = q, q + 8, ... in ascending order, then the 8
    // sums are added in ascending q -- the same in every workgroup
    const int j = tid % BD_PMAX, q = tid / BD_PMAX;
    double s = 0.0;
    if (j < p)
      for (int g = q; g < G; g += BD_FOLD) s += part[(int64_t)g * p + j];
    fold[q * BD_PMAX + j] = s;
  }
  __syncthreads();
  if (tid < IPX_WAVE) {                                       // wave 0, every lane active
    const int lane = tid;
    double ti = 0.0;
    if (lane < p) {
      ti = fold[lane];
      for (int q = 1; q < BD_FOLD; ++q) ti += fold[q * BD_PMAX + lane];
    }
    for (int k = 0; k < p; ++k) {                             // L y = t
      const double yk = __shfl(ti, k) / Ls[k * BD_PAD + k];
      if (lane == k) ti = yk;
      else if (lane > k && lane < p) ti = __builtin_fma(-Ls[lane * BD_PAD + k], yk, ti);
    }
    for (int k = p - 1; k >= 0; --k) {                        // L' z = y
      const double zk = __shfl(ti, k) / Ls[k * BD_PAD + k];
      if (lane == k) ti = zk;
      else if (lane < k) ti = __builtin_fma(-Ls[k * BD_PAD + lane], zk, ti);
    }
    if (lane < p) z[lane] = ti;
  }
  __syncthreads();
  const int64_t chunks = bd_chunks(m);
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const int64_t r = c * BD_ROWS + tid;
    if (r < m) {
      double acc = u[r];
      for (int j = 0; j < p; ++j) acc = __builtin_fma(-Y[r + m * j], z[j], acc);
      v[r] = acc;
    }
  }
}

inline bool bd_valid(int64_t m, int32_t p) {
  return m >= 1 && p >= 1 && p <= BD_PMAX && m <= (int64_t)INT32_MAX - BD_ROWS;
}

}  // namespace

extern "C" {

int ipx_border_pmax(void) { return BD_PMAX; }

int ipx_border_rows_per_group(void) { return BD_ROWS; }

int ipx_border_groups(int64_t m) { return m < 1 ? IPX_EINVAL : bd_groups(m); }

int ipx_border_scatter(int64_t m, int32_t p, int64_t nnz, const double *val, const int32_t *src,
                       const int64_t *dst, double *C, void *stream) {
  if (!bd_valid(m, p) || nnz < 0 || nnz > m * p || !C || (nnz && (!val || !src || !dst)))
    return IPX_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = m * p;
  hipLaunchKernelGGL(k_bd_fill, dim3((unsigned)((n + IPX_BLOCK - 1) / IPX_BLOCK)),
                     dim3(IPX_BLOCK), 0, st, n, C);
  IPX_CHECK_LAUNCH();
  if (nnz) {
    hipLaunchKernelGGL(k_bd_scatter, dim3((unsigned)((nnz + IPX_BLOCK - 1) / IPX_BLOCK)),
                       dim3(IPX_BLOCK), 0, st, nnz, val, src, dst, C);
    IPX_CHECK_LAUNCH();
  }
  return IPX_OK;
}

int ipx_border_gram(int64_t m, int32_t p, const double *C, const double *Y, double *part,
                    void *stream) {
  if (!bd_valid(m, p) || !C || !Y || !part) return IPX_EINVAL;
  hipLaunchKernelGGL(k_bd_gram_partial, dim3(bd_groups(m)), dim3(IPX_BLOCK), 0,
                     (hipStream_t)stream, m, (int)p, C, Y, part);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

int ipx_border_chol(int64_t m, int32_t p, const double *part, double *K, double *L, double *info,
                    void *stream) {
  if (!bd_valid(m, p) || !part || !K || !L || !info) return IPX_EINVAL;
  hipLaunchKernelGGL(k_bd_chol, dim3(1), dim3(IPX_BLOCK), 0, (hipStream_t)stream, (int)p,
                     bd_groups(m), part, K, L, info);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

int ipx_border_tdot(int64_t m, int32_t p, const double *Y, const double *w, double *part,
                    void *stream) {
  if (!bd_valid(m, p) || !Y || !w || !part) return IPX_EINVAL;
  hipLaunchKernelGGL(k_bd_tdot, dim3(bd_groups(m)), dim3(IPX_BLOCK), 0, (hipStream_t)stream, m,
                     (int)p, Y, w, part);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

int ipx_border_apply(int64_t m, int32_t p, const double *Y, const double *L, const double *part,
                     const double *u, double *v, void *stream) {
  if (!bd_valid(m, p) || !Y || !L || !part || !u || !v) return IPX_EINVAL;
  const int64_t chunks = bd_chunks(m);
  const int grid = (int)(chunks < BD_APPLY_CAP ? chunks : BD_APPLY_CAP);
  hipLaunchKernelGGL(k_bd_apply, dim3(grid), dim3(IPX_BLOCK), 0, (hipStream_t)stream, m, (int)p,
                     bd_groups(m), Y, L, part, u, v);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

}  // extern "C"
