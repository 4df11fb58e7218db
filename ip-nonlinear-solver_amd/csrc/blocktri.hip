// Block-tridiagonal direct (A A')^-1 by block cyclic reduction, for half bandwidths past the
// banded solver's (csrc/banded.hip, k <= 8) up to 64 -- and, in the second part of this file
// (ipx_blockwide_*: blocks of 128 and 256 worked on as tiles of 64 x 64), up to 256.
//
// S = P A A' P' with half bandwidth k <= b is block tridiagonal in blocks of b (16, 32, 64):
// N = ceil(m / b) block rows, D_I = S[I, I] and E_I = S[I, I - 1]; the padded tail rows carry a
// unit diagonal.  A level of the reduction (stride s = 1, 2, 4, ...: the surviving block rows
// are the multiples of s, numbered i = I / s) eliminates the odd ones.  For an odd row J with
// its neighbours J - s and J + s:
//     D_J = L_J L_J'              (Cholesky; no pivoting: every Schur complement of an SPD
//                                  matrix is SPD)
//     U_J = L_J^-1 E_J            (coupling to J - s)
//     V_J = L_J^-1 E_{J+s}'       (coupling to J + s)
// and for an even row I (the survivors):
//     D_I  <- D_I - V_{I-s}' V_{I-s} - U_{I+s}' U_{I+s}
//     E_I  <- - V_{I-s}' U_{I-s}                       (now the coupling of I to I - 2 s)
// L, U, V are exactly the block columns of the Cholesky factor of S in odd-even order, so the
// solve applies TRIANGULAR FACTORS (two b x b triangular solves per pivot block), never an
// inverse: backward stable as any Cholesky factorization, at the price of b dependent steps per
// block.  Right-hand side: y_J = L_J^-1 r_J, r_{J-s} -= U_J' y_J,
// r_{J+s} -= V_J' y_J down the levels; x_J = L_J^-T (y_J - U_J x_{J-s} - V_J x_{J+s}) up.
//
// Storage: every block row is eliminated exactly once, so everything lives at the ORIGINAL
// block index and the factorization runs in place: ws = [D | E | V | diag0 | r | y] with D, E, V
// N b^2 doubles each (L_J over D_J, U_J over E_J) and diag0, r, y N b doubles (the diagonal
// before the factorization, for the pivot test; the solve's two work vectors).  Python owns ws;
// nothing is allocated here.
//
// Launches: a level is two launches in the factorization (the odd rows, then the even rows --
// an even row takes the products of both its neighbours in a fixed order, no atomics) and one
// per direction in the solve.  Once ceil(N / s) <= 512 / b block rows survive, ONE workgroup
// finishes all remaining levels in a single launch, its blocks staged through LDS.
// The b x b x b products (V'V, U'U, V'U) run on v_mfma_f64_16x16x4_f64 (operand layout: lane l
// supplies A element (row l & 15, k l >> 4), B element (k l >> 4, col l & 15); D: col l & 15,
// row (l >> 4) + 4 reg -- as csrc/dense.hip).  Everything is fixed-order fp64; square roots and
// divisions are the correctly rounded ones, so a matrix scaled by 4^s factors to the same bits
// times 2^s and an exactly singular integer block gives an exactly zero pivot.
// Pivot signals (flag, relative only): bit 0 -- a pivot lost 43 bits against its original
// diagonal entry (IPX_PIVOT_RTOL); bits 0 and 2 -- a pivot <= 0 (the factorization goes on with
// 1 in its place: nothing faults, the result is refused by the caller).
#include "ipx_common.h"

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int BT_KMAX = 64;
constexpr int BT_TAIL_ROWS = 512;          // the one-workgroup tail takes over at <= 512 / b block rows
constexpr int BT_SOLVE_BLOCK = IPX_WAVE;   // the solve: a wave per block row

struct BtStore {
  double *D, *E, *V, *diag0, *r, *y;
};

inline BtStore bt_store(double *ws, int64_t N, int b) {
  BtStore S;
  const int64_t blk = N * b * b, vec = N * b;
  S.D = ws;
  S.E = ws + blk;
  S.V = ws + 2 * blk;
  S.diag0 = ws + 3 * blk;
  S.r = S.diag0 + vec;
  S.y = S.r + vec;
  return S;
}

inline bool bt_valid_b(int b) { return b == 16 || b == 32 || b == 64; }

// ------------------------------------------------------------------------------ assembly
// merge join of two sorted CSR rows, products added in the order of the columns (banded.hip)
__device__ __forceinline__ double bt_join(int p, int pe, int u, int ue,
                                          const int32_t *__restrict__ col,
                                          const double *__restrict__ val) {
  double s = 0.0;
  while (p < pe && u < ue) {
    const int cp = col[p], cu = col[u];
    if (cp == cu) { s += val[p] * val[u]; ++p; ++u; }
    else if (cp < cu) ++p;
    else ++u;
  }
  return s;
}

// one lane per entry of D (which = 0) and E (which = 1)
__global__ void __launch_bounds__(IPX_BLOCK)
k_bt_aat(int m, int b, int k, int64_t N, const int32_t *__restrict__ rowptr,
         const int32_t *__restrict__ colidx, const double *__restrict__ val,
         const int32_t *__restrict__ perm, double *__restrict__ D, double *__restrict__ E) {
  const int64_t blk = N * b * b;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 2 * blk) return;
  const int which = idx >= blk;
  const int64_t e = idx - which * blk;
  const int64_t I = e / (b * b);
  const int rc = (int)(e - I * b * b), r = rc / b, c = rc - r * b;
  const int64_t i = I * b + r, j = (I - which) * b + c;
  double v = 0.0;
  if (i < m && j < m && j >= 0) {
    const int64_t dist = i > j ? i - j : j - i;
    if (dist <= k) {
      const int r1 = perm ? perm[i] : (int)i, r2 = perm ? perm[j] : (int)j;
      v = bt_join(rowptr[r1], rowptr[r1 + 1], rowptr[r2], rowptr[r2 + 1], colidx, val);
    }
  } else if (!which && i >= m && i == j) {
    v = 1.0;                                          // padded tail: unit diagonal
  }
  (which ? E : D)[e] = v;
}

// ------------------------------------------------------------------- factorization steps
// LDS of a step, doubles: eliminate T[b][b+1] + R[b][2b+1] + col[b]; update 2 x [b][b+1]
constexpr size_t bt_factor_lds(int b) {
  return sizeof(double) * ((size_t)b * (b + 1) + (size_t)b * (2 * b + 1) + b);
}
constexpr size_t bt_update_lds(int b) { return sizeof(double) * 2 * (size_t)b * (b + 1); }

// Odd row J at stride s by one workgroup: D_J -> L_J, E_J -> U_J, V_J.
template <int B>
__device__ void bt_eliminate(double *sm, const BtStore &S, int N, int J, int s, int *flag) {
  constexpr int P = B + 1, PR = 2 * B + 1;
  double *T = sm, *R = sm + B * P, *colv = R + B * PR;
  const int tid = threadIdx.x;
  const bool hasU = J - s >= 0, hasV = J + s < N;
  double *Dj = S.D + (int64_t)J * B * B;
  double *Ej = S.E + (int64_t)J * B * B;
  double *Vj = S.V + (int64_t)J * B * B;
  const double *Ei = S.E + (int64_t)(hasV ? J + s : J) * B * B;
  __syncthreads();                                    // (the tail: the previous step's LDS)
  for (int e = tid; e < B * B; e += IPX_BLOCK) {
    const int r = e / B, c = e % B;
    T[r * P + c] = Dj[e];
    R[r * PR + c] = hasU ? Ej[e] : 0.0;
    R[c * PR + B + r] = hasV ? Ei[e] : 0.0;           // E_{J+s}' (transposed on the way in)
  }
  __syncthreads();
  // right-looking Cholesky, a column per trip: the scaled column goes through colv
  int bits = 0;
  for (int j = 0; j < B; ++j) {
    const double d = T[j * P + j];
    if (tid == 0) {
      const double d0 = S.diag0[(int64_t)J * B + j];
      if (!(d > IPX_PIVOT_RTOL * d0)) bits |= (d > 0.0) ? 1 : 5;
    }
    const double l = sqrt(d > 0.0 ? d : 1.0);
    if (tid >= j && tid < B) colv[tid] = tid == j ? l : T[tid * P + j] / l;
    __syncthreads();
    const int rem = B - j - 1;
    for (int e = tid; e < rem * rem; e += IPX_BLOCK) {
      const int i = j + 1 + e / rem, c = j + 1 + e % rem;
      if (c <= i) T[i * P + c] = __builtin_fma(-colv[i], colv[c], T[i * P + c]);
    }
    if (tid >= j && tid < B) T[tid * P + j] = colv[tid];
    __syncthreads();
  }
  // L X = [E_J | E_{J+s}']: a lane per right-hand-side column, forward substitution in place
  if (tid < 2 * B && (tid < B ? hasU : hasV)) {
    const int c = tid;
    for (int k = 0; k < B; ++k) {
      double acc = R[k * PR + c];
#pragma unroll 8
      for (int q = 0; q < k; ++q) acc = __builtin_fma(-T[k * P + q], R[q * PR + c], acc);
      R[k * PR + c] = acc / T[k * P + k];
    }
  }
  __syncthreads();
  for (int e = tid; e < B * B; e += IPX_BLOCK) {
    const int r = e / B, c = e % B;
    Dj[e] = c <= r ? T[r * P + c] : 0.0;
    if (hasU) Ej[e] = R[r * PR + c];
    if (hasV) Vj[e] = R[r * PR + B + c];
  }
  if (tid == 0 && bits) atomicOr(flag, bits);
}

// Even row I at stride s by one workgroup: the Schur complement's blocks, on the matrix cores.
// The 2 (B/16)^2 output tiles (D's, then E's) are dealt to the four waves round robin.
template <int B>
__device__ void bt_update(double *sm, const BtStore &S, int N, int I, int s) {
  constexpr int P = B + 1, TB = B / 16, TT = TB * TB, NTW = (2 * TT + 3) / 4;
  double *Pm = sm, *Qm = sm + B * P;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const bool hasL = I - s >= 0, hasR = I + s < N;
  v4d acc[NTW];
#pragma unroll
  for (int u = 0; u < NTW; ++u) acc[u] = (v4d){0.0, 0.0, 0.0, 0.0};
  __syncthreads();
  if (hasL) {
    const double *Vl = S.V + (int64_t)(I - s) * B * B, *Ul = S.E + (int64_t)(I - s) * B * B;
    for (int e = tid; e < B * B; e += IPX_BLOCK) {
      Pm[(e / B) * P + e % B] = Vl[e];
      Qm[(e / B) * P + e % B] = Ul[e];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NTW; ++u) {
      const int id = wave + 4 * u;
      if (id < 2 * TT) {
        const bool isE = id >= TT;
        const int t = isE ? id - TT : id, tr = t / TB, tc = t % TB;
        const double *pa = Pm + lk * P + 16 * tr + lr;
        const double *pb = (isE ? Qm : Pm) + lk * P + 16 * tc + lr;
#pragma unroll 4
        for (int k0 = 0; k0 < B; k0 += 4)
          acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[k0 * P], pb[k0 * P], acc[u], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  if (hasR) {
    const double *Ur = S.E + (int64_t)(I + s) * B * B;
    for (int e = tid; e < B * B; e += IPX_BLOCK) Pm[(e / B) * P + e % B] = Ur[e];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NTW; ++u) {
      const int id = wave + 4 * u;
      if (id < TT) {
        const int tr = id / TB, tc = id % TB;
        const double *pa = Pm + lk * P + 16 * tr + lr;
        const double *pb = Pm + lk * P + 16 * tc + lr;
#pragma unroll 4
        for (int k0 = 0; k0 < B; k0 += 4)
          acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[k0 * P], pb[k0 * P], acc[u], 0, 0, 0);
      }
    }
  }
  double *Di = S.D + (int64_t)I * B * B, *Ei = S.E + (int64_t)I * B * B;
#pragma unroll
  for (int u = 0; u < NTW; ++u) {
    const int id = wave + 4 * u;
    if (id < 2 * TT) {
      const bool isE = id >= TT;
      const int t = isE ? id - TT : id, tr = t / TB, tc = t % TB;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int at = (16 * tr + lk + 4 * g) * B + 16 * tc + lr;
        if (!isE) Di[at] -= acc[u][g];
        else if (hasL) Ei[at] = -acc[u][g];
      }
    }
  }
}

template <int B>
__global__ void __launch_bounds__(IPX_BLOCK) k_bt_eliminate(BtStore S, int N, int s, int *flag) {
  extern __shared__ __attribute__((aligned(16))) double bt_sm[];
  bt_eliminate<B>(bt_sm, S, N, (2 * (int)blockIdx.x + 1) * s, s, flag);
}

template <int B>
__global__ void __launch_bounds__(IPX_BLOCK) k_bt_update(BtStore S, int N, int s) {
  extern __shared__ __attribute__((aligned(16))) double bt_sm[];
  bt_update<B>(bt_sm, S, N, 2 * (int)blockIdx.x * s, s);
}

// Every level from stride s on, and the last block's Cholesky, by one workgroup.  What a step
// leaves in global memory the next one reads after a barrier (one workgroup: one CU's cache).
template <int B>
__global__ void __launch_bounds__(IPX_BLOCK) k_bt_factor_tail(BtStore S, int N, int s, int *flag) {
  extern __shared__ __attribute__((aligned(16))) double bt_sm[];
  int n = (N + s - 1) / s;
  while (n > 1) {
    for (int t = 0; t < n / 2; ++t) bt_eliminate<B>(bt_sm, S, N, (2 * t + 1) * s, s, flag);
    for (int t = 0; t < (n + 1) / 2; ++t) bt_update<B>(bt_sm, S, N, 2 * t * s, s);
    s *= 2;
    n = (n + 1) / 2;
  }
  bt_eliminate<B>(bt_sm, S, N, 0, s, flag);           // (s >= N: neither neighbour)
}

// D, E into the store (unless they are the store), the diagonal aside, the flag cleared
__global__ void __launch_bounds__(IPX_BLOCK)
k_bt_begin(int64_t N, int b, const double *D, const double *E, BtStore S, int *flag) {
  const int64_t blk = N * b * b;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx == 0) *flag = 0;
  if (idx >= blk) return;
  const double d = D[idx];
  if (D != S.D) { S.D[idx] = d; S.E[idx] = E[idx]; }
  const int64_t I = idx / (b * b);
  const int rc = (int)(idx - I * b * b), r = rc / b, c = rc - r * b;
  if (r == c) S.diag0[I * b + r] = d;
}

template <int B>
int bt_factor(int64_t N, const double *D, const double *E, double *ws, int *flag, hipStream_t st) {
  const BtStore S = bt_store(ws, N, B);
  const size_t lds = bt_factor_lds(B);
  // the dynamic-LDS limit (99.8 KB at B = 64) is raised at every call, for the device that is
  // current now -- three host calls against the 2 + 2 l0 launches below -- and a refusal is
  // this call's error, not a later launch's
  hipError_t e = hipFuncSetAttribute((const void *)k_bt_eliminate<B>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e == hipSuccess)
    e = hipFuncSetAttribute((const void *)k_bt_update<B>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)bt_update_lds(B));
  if (e == hipSuccess)
    e = hipFuncSetAttribute((const void *)k_bt_factor_tail<B>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) {
    ipx_note_error(e, __FILE__, __LINE__);
    return IPX_ELAUNCH;
  }
  const int64_t blk = N * B * B;
  hipLaunchKernelGGL(k_bt_begin, dim3((unsigned)((blk + IPX_BLOCK - 1) / IPX_BLOCK)),
                     dim3(IPX_BLOCK), 0, st, N, B, D, E, S, flag);
  IPX_CHECK_LAUNCH();
  int s = 1, n = (int)N;
  while (n > BT_TAIL_ROWS / B) {
    hipLaunchKernelGGL(k_bt_eliminate<B>, dim3(n / 2), dim3(IPX_BLOCK), lds, st, S, (int)N, s,
                       flag);
    IPX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_bt_update<B>, dim3((n + 1) / 2), dim3(IPX_BLOCK), bt_update_lds(B), st, S,
                       (int)N, s);
    IPX_CHECK_LAUNCH();
    s *= 2;
    n = (n + 1) / 2;
  }
  hipLaunchKernelGGL(k_bt_factor_tail<B>, dim3(1), dim3(IPX_BLOCK), lds, st, S, (int)N, s, flag);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

// ---------------------------------------------------------------------------- solve steps
// A wave per block row; lane c holds entry c of a b-vector (lanes >= B idle along).
template <int B>
__device__ __forceinline__ void bt_stage(double *M, const double *src, int lane) {
  constexpr int P = B + 1;
  __syncthreads();
  for (int e = lane; e < B * B; e += BT_SOLVE_BLOCK) M[(e / B) * P + e % B] = src[e];
  __syncthreads();
}

// y = L^-1 v (L staged in M), right-looking: y_q travels by v_readlane
template <int B>
__device__ __forceinline__ double bt_lower(const double *M, double v, int lane) {
  constexpr int P = B + 1;
  for (int q = 0; q < B; ++q) {
    const double yq = ipx_readlane(v, q) / M[q * P + q];
    if (lane == q) v = yq;
    else if (lane > q && lane < B) v = __builtin_fma(-M[lane * P + q], yq, v);
  }
  return v;
}

// x = L^-T v
template <int B>
__device__ __forceinline__ double bt_upper(const double *M, double v, int lane) {
  constexpr int P = B + 1;
  for (int q = B - 1; q >= 0; --q) {
    const double xq = ipx_readlane(v, q) / M[q * P + q];
    if (lane == q) v = xq;
    else if (lane < q) v = __builtin_fma(-M[q * P + lane], xq, v);
  }
  return v;
}

// (G' y)_lane, G a b x b block in global memory (rows read across the lanes)
template <int B>
__device__ __forceinline__ double bt_tmatvec(const double *G, double y, int lane) {
  double acc = 0.0;
  const int c = lane < B ? lane : 0;
#pragma unroll 4
  for (int k = 0; k < B; ++k) acc = __builtin_fma(G[k * B + c], ipx_readlane(y, k), acc);
  return acc;
}

// (M x)_lane, M staged in LDS
template <int B>
__device__ __forceinline__ double bt_matvec(const double *M, double x, int lane) {
  constexpr int P = B + 1;
  double acc = 0.0;
  const int r = lane < B ? lane : 0;
#pragma unroll 4
  for (int c = 0; c < B; ++c) acc = __builtin_fma(M[r * P + c], ipx_readlane(x, c), acc);
  return acc;
}

// Even row I at stride s: r_I -= V_{I-s}' y_{I-s} + U_{I+s}' y_{I+s}, y = L^-1 r of the odd
// neighbours (both computed here; the one to the right is also stored: each y is written once,
// by its left neighbour's wave).
template <int B>
__device__ void bt_forward(double *M, const BtStore &S, int N, int I, int s) {
  const int lane = threadIdx.x;
  const bool on = lane < B;
  double rI = on ? S.r[(int64_t)I * B + lane] : 0.0;
  if (I - s >= 0) {
    const int64_t J = I - s;
    bt_stage<B>(M, S.D + J * B * B, lane);
    const double y = bt_lower<B>(M, on ? S.r[J * B + lane] : 0.0, lane);
    rI -= bt_tmatvec<B>(S.V + J * B * B, y, lane);
  }
  if (I + s < N) {
    const int64_t J = I + s;
    bt_stage<B>(M, S.D + J * B * B, lane);
    const double y = bt_lower<B>(M, on ? S.r[J * B + lane] : 0.0, lane);
    if (on) S.y[J * B + lane] = y;
    rI -= bt_tmatvec<B>(S.E + J * B * B, y, lane);
  }
  if (on) S.r[(int64_t)I * B + lane] = rI;
}

// entry `lane` of block row I of x (zero in the padded tail, which x does not have)
template <int B>
__device__ __forceinline__ double bt_x_at(const double *x, int m, int64_t I, int lane) {
  const int64_t i = I * B + lane;
  return (lane < B && i < m) ? x[i] : 0.0;
}

// Odd row J at stride s: x_J = L_J^-T (y_J - U_J x_{J-s} - V_J x_{J+s})
template <int B>
__device__ void bt_back(double *M, const BtStore &S, int N, int J, int s, double *x, int m) {
  const int lane = threadIdx.x;
  double v = lane < B ? S.y[(int64_t)J * B + lane] : 0.0;
  if (J - s >= 0) {
    bt_stage<B>(M, S.E + (int64_t)J * B * B, lane);
    v -= bt_matvec<B>(M, bt_x_at<B>(x, m, J - s, lane), lane);
  }
  if (J + s < N) {
    bt_stage<B>(M, S.V + (int64_t)J * B * B, lane);
    v -= bt_matvec<B>(M, bt_x_at<B>(x, m, J + s, lane), lane);
  }
  bt_stage<B>(M, S.D + (int64_t)J * B * B, lane);
  v = bt_upper<B>(M, v, lane);
  const int64_t i = (int64_t)J * B + lane;
  if (lane < B && i < m) x[i] = v;
}

template <int B>
__global__ void __launch_bounds__(BT_SOLVE_BLOCK) k_bt_forward(BtStore S, int N, int s) {
  __shared__ double M[B * (B + 1)];
  bt_forward<B>(M, S, N, 2 * (int)blockIdx.x * s, s);
}

template <int B>
__global__ void __launch_bounds__(BT_SOLVE_BLOCK)
k_bt_back(BtStore S, int N, int s, double *x, int m) {
  __shared__ double M[B * (B + 1)];
  bt_back<B>(M, S, N, (2 * (int)blockIdx.x + 1) * s, s, x, m);
}

// The levels from stride s0 on, down and up again, by one wave
template <int B>
__global__ void __launch_bounds__(BT_SOLVE_BLOCK)
k_bt_solve_tail(BtStore S, int N, int s0, double *x, int m) {
  __shared__ double M[B * (B + 1)];
  const int lane = threadIdx.x;
  int s = s0, n = (N + s - 1) / s;
  while (n > 1) {
    for (int t = 0; t < (n + 1) / 2; ++t) bt_forward<B>(M, S, N, 2 * t * s, s);
    s *= 2;
    n = (n + 1) / 2;
  }
  bt_stage<B>(M, S.D, lane);                          // the last block: row 0
  double v = bt_lower<B>(M, lane < B ? S.r[lane] : 0.0, lane);
  v = bt_upper<B>(M, v, lane);
  if (lane < B && lane < m) x[lane] = v;
  while (s > s0) {
    s /= 2;
    n = (N + s - 1) / s;
    for (int t = 0; t < n / 2; ++t) bt_back<B>(M, S, N, (2 * t + 1) * s, s, x, m);
  }
}

__global__ void __launch_bounds__(IPX_BLOCK)
k_bt_rhs(int64_t len, int m, const double *__restrict__ w, double *__restrict__ r) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < len) r[i] = i < m ? w[i] : 0.0;
}

template <int B>
int bt_solve(int64_t m, int64_t N, double *ws, const double *w, double *x, hipStream_t st) {
  const BtStore S = bt_store(ws, N, B);
  hipLaunchKernelGGL(k_bt_rhs, dim3((unsigned)((N * B + IPX_BLOCK - 1) / IPX_BLOCK)),
                     dim3(IPX_BLOCK), 0, st, N * B, (int)m, w, S.r);
  IPX_CHECK_LAUNCH();
  int s = 1, n = (int)N;
  while (n > BT_TAIL_ROWS / B) {
    hipLaunchKernelGGL(k_bt_forward<B>, dim3((n + 1) / 2), dim3(BT_SOLVE_BLOCK), 0, st, S, (int)N,
                       s);
    IPX_CHECK_LAUNCH();
    s *= 2;
    n = (n + 1) / 2;
  }
  hipLaunchKernelGGL(k_bt_solve_tail<B>, dim3(1), dim3(BT_SOLVE_BLOCK), 0, st, S, (int)N, s, x,
                     (int)m);
  IPX_CHECK_LAUNCH();
  while (s > 1) {
    s /= 2;
    n = (int)((N + s - 1) / s);
    hipLaunchKernelGGL(k_bt_back<B>, dim3(n / 2), dim3(BT_SOLVE_BLOCK), 0, st, S, (int)N, s, x,
                       (int)m);
    IPX_CHECK_LAUNCH();
  }
  return IPX_OK;
}

// =============================================================================================
// Wide blocks: b = 128, 256 (half bandwidths 65 ... 256).  The same
// reduction, the same storage, the same pivot signals -- but a block (128 / 512 KiB) no longer
// fits in LDS, so every step works on the T x T tiles of 64 x 64 of a block (T = b / 64), the
// blocks themselves staying in global memory:
//   a level of the factorization is three launches --
//     k_bw_chol    a workgroup per odd row: blocked right-looking Cholesky of D_J in place (the
//                  diagonal tile by bt_eliminate's column loop in LDS, the panel under it a
//                  triangular solve per tile row out of LDS, the trailing tiles on the matrix cores);
//     k_bw_trsm    (odd rows) x (2 T strips of 64 columns of [E_J | E_{J+s}']): forward
//                  substitution tile row by tile row, sum_{q<i} L_iq X_q on the matrix cores,
//                  the 64 x 64 triangular part out of LDS;
//     k_bw_schur   (even rows) x (2 T^2 output tiles of D_I and E_I): a K = b (D: 2 b, V'V then
//                  U'U) accumulation on the matrix cores, written once;
//   the last block is one more k_bw_chol; there is no one-workgroup tail (a level's work is
//   far past a launch at these sizes).  The solve is one launch per level and direction, a
//   workgroup per block row, the triangular solves 64 rows at a time through LDS.
// A workgroup reads what it wrote itself to global memory only after a barrier (as the tail of
// the narrow solver does).  MFMA operands come straight from global memory (L2-resident: a
// workgroup's operands are at most 3 b^2 doubles).
constexpr int BW_KMAX = 256;
constexpr int BW_TILE = 64;
constexpr int BW_P = BW_TILE + 1;                      // LDS row pitch of a tile

inline bool bw_valid_b(int b) { return b == 128 || b == 256; }

// A wave's 16 x 64 share of a 64 x 64 product, K deep, on v_mfma_f64_16x16x4_f64:
//   acc[tc] (rows 16 wave + ..., columns 16 tc + ...) += sum_k A(row, k) Bm(k, col).
// pa points at A(16 wave + (lane & 15), lane >> 4), one k is sa_k doubles further; pb at
// Bm(lane >> 4, lane & 15), one k is sb_k, sixteen columns are sb_16 doubles further.
__device__ __forceinline__ void bw_mma(v4d (&acc)[4], const double *pa, int64_t sa_k,
                                       const double *pb, int64_t sb_k, int64_t sb_16, int K) {
  for (int k0 = 0; k0 < K; k0 += 4) {
    const double a = pa[k0 * sa_k];
    const double b0 = pb[k0 * sb_k], b1 = pb[k0 * sb_k + sb_16];
    const double b2 = pb[k0 * sb_k + 2 * sb_16], b3 = pb[k0 * sb_k + 3 * sb_16];
    acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b0, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b1, acc[1], 0, 0, 0);
    acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b2, acc[2], 0, 0, 0);
    acc[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b3, acc[3], 0, 0, 0);
  }
}

__device__ __forceinline__ void bw_zero(v4d (&acc)[4]) {
#pragma unroll
  for (int u = 0; u < 4; ++u) acc[u] = (v4d){0.0, 0.0, 0.0, 0.0};
}

// LDS of k_bw_chol: the diagonal tile, the T - 1 panel tiles under it, the scaled column
constexpr size_t bw_chol_lds(int b) {
  return sizeof(double) * ((size_t)(b / BW_TILE) * BW_TILE * BW_P + BW_TILE);
}
constexpr size_t bw_trsm_lds() { return sizeof(double) * 2 * BW_TILE * BW_P; }

// Row J0 + 2 s blockIdx.x: D_J = L_J L_J' in place (the strict upper triangle zeroed).
template <int B>
__global__ void __launch_bounds__(IPX_BLOCK) k_bw_chol(BtStore S, int J0, int s, int *flag) {
  constexpr int T = B / BW_TILE, P = BW_P;
  extern __shared__ __attribute__((aligned(16))) double bt_sm[];
  double *Lk = bt_sm, *Pn = bt_sm + BW_TILE * P, *colv = bt_sm + T * BW_TILE * P;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int64_t J = J0 + 2 * (int64_t)s * blockIdx.x;
  double *Dj = S.D + J * B * B;
  const double *d0 = S.diag0 + J * B;
  int bits = 0;
  for (int kt = 0; kt < T; ++kt) {
    const int below = T - 1 - kt;                     // tile rows under the diagonal tile
    __syncthreads();                                  // (the previous trip's updates, its LDS)
    for (int e = tid; e < (below + 1) * BW_TILE * BW_TILE; e += IPX_BLOCK) {
      const int r = e >> 6, c = e & 63;               // r: row under the top of the diagonal tile
      bt_sm[r * P + c] = Dj[(int64_t)(BW_TILE * kt + r) * B + BW_TILE * kt + c];
    }
    __syncthreads();
    // the diagonal tile: bt_eliminate's column loop
    for (int j = 0; j < BW_TILE; ++j) {
      const double d = Lk[j * P + j];
      if (tid == 0) {
        const double dd = d0[BW_TILE * kt + j];
        if (!(d > IPX_PIVOT_RTOL * dd)) bits |= (d > 0.0) ? 1 : 5;
      }
      const double l = sqrt(d > 0.0 ? d : 1.0);
      if (tid >= j && tid < BW_TILE) colv[tid] = tid == j ? l : Lk[tid * P + j] / l;
      __syncthreads();
      const int rem = BW_TILE - j - 1;
      for (int e = tid; e < rem * rem; e += IPX_BLOCK) {
        const int i = j + 1 + e / rem, c = j + 1 + e % rem;
        if (c <= i) Lk[i * P + c] = __builtin_fma(-colv[i], colv[c], Lk[i * P + c]);
      }
      if (tid >= j && tid < BW_TILE) Lk[tid * P + j] = colv[tid];
      __syncthreads();
    }
    // the panel: X L_kk' = A, a lane per row (rows of the tiles under the diagonal tile)
    if (tid < below * BW_TILE) {
      double *x = Pn + tid * P;
      for (int c = 0; c < BW_TILE; ++c) {
        double acc = x[c];
#pragma unroll 8
        for (int q = 0; q < c; ++q) acc = __builtin_fma(-x[q], Lk[c * P + q], acc);
        x[c] = acc / Lk[c * P + c];
      }
    }
    __syncthreads();
    for (int e = tid; e < (below + 1) * BW_TILE * BW_TILE; e += IPX_BLOCK) {
      const int r = e >> 6, c = e & 63;
      Dj[(int64_t)(BW_TILE * kt + r) * B + BW_TILE * kt + c] =
          (r >= BW_TILE || c <= r) ? bt_sm[r * P + c] : 0.0;
    }
    for (int e = tid; e < below * BW_TILE * BW_TILE; e += IPX_BLOCK) {   // tiles right of it: zero
      const int r = e / (below * BW_TILE), c = e % (below * BW_TILE);
      Dj[(int64_t)(BW_TILE * kt + r) * B + BW_TILE * (kt + 1) + c] = 0.0;
    }
    // the trailing tiles (i, j), kt < j <= i: A_ij -= L_i,kt L_j,kt' (operands: the panel in LDS)
    for (int ti = 0; ti < below; ++ti) {
      for (int tj = 0; tj <= ti; ++tj) {
        v4d acc[4];
        bw_zero(acc);
        bw_mma(acc, Pn + (ti * BW_TILE + 16 * wave + lr) * P + lk, 1,
               Pn + (tj * BW_TILE + lr) * P + lk, 1, 16 * P, BW_TILE);
        double *c = Dj + (int64_t)(BW_TILE * (kt + 1 + ti)) * B + BW_TILE * (kt + 1 + tj);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
          for (int g = 0; g < 4; ++g)
            c[(int64_t)(16 * wave + lk + 4 * g) * B + 16 * u + lr] -= acc[u][g];
        }
      }
    }
  }
  if (tid == 0 && bits) atomicOr(flag, bits);
}

// Odd row J at stride s, strip blockIdx.y of [E_J | E_{J+s}']: U_J (strips < T, in place) and
// V_J (strips >= T) by forward substitution with L_J, a tile row at a time.
template <int B>
__global__ void __launch_bounds__(IPX_BLOCK) k_bw_trsm(BtStore S, int N, int s) {
  constexpr int T = B / BW_TILE, P = BW_P;
  extern __shared__ __attribute__((aligned(16))) double bt_sm[];
  double *Lk = bt_sm, *R = bt_sm + BW_TILE * P;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int64_t J = (2 * (int64_t)blockIdx.x + 1) * s;
  const bool isV = (int)blockIdx.y >= T;
  const int c0 = BW_TILE * ((int)blockIdx.y - (isV ? T : 0));
  if (isV ? J + s >= N : J - s < 0) return;
  const double *Lj = S.D + J * B * B;
  const double *src = S.E + (isV ? J + s : J) * B * B;
  double *out = (isV ? S.V : S.E) + J * B * B;
  for (int i = 0; i < T; ++i) {
    v4d acc[4];
    bw_zero(acc);
    __syncthreads();                                  // (the rows this workgroup stored before)
    // sum_{q < i} L_iq X_q: K = 64 i, X from where it was stored
    bw_mma(acc, Lj + (int64_t)(BW_TILE * i + 16 * wave + lr) * B + lk, 1,
           out + (int64_t)lk * B + c0 + lr, B, 16, BW_TILE * i);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int r = 16 * wave + lk + 4 * g, c = 16 * u + lr;
        const int64_t row = BW_TILE * i + r, col = c0 + c;
        const double a = isV ? src[col * B + row] : src[row * B + col];
        R[r * P + c] = a - acc[u][g];
      }
    }
    for (int e = tid; e < BW_TILE * BW_TILE; e += IPX_BLOCK) {
      const int r = e >> 6, c = e & 63;
      Lk[r * P + c] = Lj[(int64_t)(BW_TILE * i + r) * B + BW_TILE * i + c];
    }
    __syncthreads();
    if (tid < BW_TILE) {                              // a lane per right-hand-side column
      for (int k = 0; k < BW_TILE; ++k) {
        double a = R[k * P + tid];
#pragma unroll 8
        for (int q = 0; q < k; ++q) a = __builtin_fma(-Lk[k * P + q], R[q * P + tid], a);
        R[k * P + tid] = a / Lk[k * P + k];
      }
    }
    __syncthreads();
    for (int e = tid; e < BW_TILE * BW_TILE; e += IPX_BLOCK) {
      const int r = e >> 6, c = e & 63;
      out[(int64_t)(BW_TILE * i + r) * B + c0 + c] = R[r * P + c];
    }
  }
}

// Even row I at stride s, output tile blockIdx.y (the T^2 of D_I, then the T^2 of E_I):
//   D_I -= V_{I-s}' V_{I-s} + U_{I+s}' U_{I+s} (one accumulator, in that order),
//   E_I = - V_{I-s}' U_{I-s}.
template <int B>
__global__ void __launch_bounds__(IPX_BLOCK) k_bw_schur(BtStore S, int N, int s) {
  constexpr int T = B / BW_TILE, TT = T * T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int64_t I = 2 * (int64_t)blockIdx.x * s;
  const bool isE = (int)blockIdx.y >= TT;
  const int t = (int)blockIdx.y - (isE ? TT : 0), tr = t / T, tc = t % T;
  const bool hasL = I - s >= 0, hasR = I + s < N;
  if (isE && !hasL) return;
  v4d acc[4];
  bw_zero(acc);
  const int ra = BW_TILE * tr + 16 * wave + lr, cb = BW_TILE * tc + lr;
  if (hasL) {
    const double *Vl = S.V + (I - s) * B * B, *Ul = S.E + (I - s) * B * B;
    bw_mma(acc, Vl + (int64_t)lk * B + ra, B, (isE ? Ul : Vl) + (int64_t)lk * B + cb, B, 16, B);
  }
  if (hasR && !isE) {
    const double *Ur = S.E + (I + s) * B * B;
    bw_mma(acc, Ur + (int64_t)lk * B + ra, B, Ur + (int64_t)lk * B + cb, B, 16, B);
  }
  double *C = (isE ? S.E : S.D) + I * B * B;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int64_t at = (int64_t)(BW_TILE * tr + 16 * wave + lk + 4 * g) * B + BW_TILE * tc +
                         16 * u + lr;
      if (isE) C[at] = -acc[u][g];
      else C[at] -= acc[u][g];
    }
  }
}

template <int B>
int bw_factor(int64_t N, const double *D, const double *E, double *ws, int *flag, hipStream_t st) {
  constexpr int T = B / BW_TILE;
  const BtStore S = bt_store(ws, N, B);
  // (the dynamic-LDS limit is raised at every call, for the device that is current now; a
  // refusal is this call's error: bt_factor)
  hipError_t e = hipFuncSetAttribute((const void *)k_bw_chol<B>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)bw_chol_lds(B));
  if (e == hipSuccess)
    e = hipFuncSetAttribute((const void *)k_bw_trsm<B>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)bw_trsm_lds());
  if (e != hipSuccess) {
    ipx_note_error(e, __FILE__, __LINE__);
    return IPX_ELAUNCH;
  }
  const int64_t blk = N * B * B;
  hipLaunchKernelGGL(k_bt_begin, dim3((unsigned)((blk + IPX_BLOCK - 1) / IPX_BLOCK)),
                     dim3(IPX_BLOCK), 0, st, N, B, D, E, S, flag);
  IPX_CHECK_LAUNCH();
  int s = 1, n = (int)N;
  while (n > 1) {
    hipLaunchKernelGGL(k_bw_chol<B>, dim3(n / 2), dim3(IPX_BLOCK), bw_chol_lds(B), st, S, s, s,
                       flag);
    IPX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_bw_trsm<B>, dim3(n / 2, 2 * T), dim3(IPX_BLOCK), bw_trsm_lds(), st, S,
                       (int)N, s);
    IPX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_bw_schur<B>, dim3((n + 1) / 2, 2 * T * T), dim3(IPX_BLOCK), 0, st, S,
                       (int)N, s);
    IPX_CHECK_LAUNCH();
    s *= 2;
    n = (n + 1) / 2;
  }
  hipLaunchKernelGGL(k_bw_chol<B>, dim3(1), dim3(IPX_BLOCK), bw_chol_lds(B), st, S, 0, s, flag);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

// ---- the solve: a workgroup per block row, a b-vector in LDS (entry c with thread c)
template <int B>
struct BwSolveLds {
  double M[BW_TILE * BW_P];      // a diagonal tile of L
  double v[B];                   // the vector being solved with / multiplied
  double t[IPX_BLOCK];           // partial sums of a product
  double acc[B];                 // the block row's own vector
};

// out[c] (c < ncols, in sm.t[c]) = sum_{k < klen} G[k ld + c] vin[k]: thread (part, c) adds its
// contiguous share of the k in order, the parts are added in order.  klen: a multiple of 64.
template <int B>
__device__ __forceinline__ void bw_tmatvec(BwSolveLds<B> &sm, const double *G, int ld, int ncols,
                                           int klen, const double *vin) {
  const int tid = threadIdx.x;
  const int parts = IPX_BLOCK / ncols, c = tid % ncols, part = tid / ncols;
  const int share = klen / parts;
  double a = 0.0;
  const double *g = G + (int64_t)part * share * ld + c;
  __syncthreads();                  // (vin's writers; sm.t: the previous product's readers)
#pragma unroll 4
  for (int k = 0; k < share; ++k) a = __builtin_fma(g[(int64_t)k * ld], vin[part * share + k], a);
  sm.t[tid] = a;
  __syncthreads();
  if (tid < ncols) {
    double r = sm.t[tid];
    for (int p = 1; p < parts; ++p) r += sm.t[p * ncols + tid];
    sm.t[tid] = r;
  }
  __syncthreads();
}

// sm.t[r] (r < nrows) = sum_{k < klen} G[r ld + k] vin[k]: a wave per row (rows dealt round
// robin), 64 k at a time across the lanes, then the wave's fixed-order sum.
template <int B>
__device__ __forceinline__ void bw_matvec(BwSolveLds<B> &sm, const double *G, int ld, int nrows,
                                          int klen, const double *vin) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  for (int r = wave; r < nrows; r += IPX_BLOCK / IPX_WAVE) {
    double a = 0.0;
    for (int k = lane; k < klen; k += IPX_WAVE) a = __builtin_fma(G[(int64_t)r * ld + k], vin[k], a);
    a = ipx_wave_sum(a);
    if (lane == 0) sm.t[r] = a;
  }
  __syncthreads();
}

template <int B>
__device__ __forceinline__ void bw_stage_tile(BwSolveLds<B> &sm, const double *L, int i) {
  __syncthreads();
  for (int e = threadIdx.x; e < BW_TILE * BW_TILE; e += IPX_BLOCK)
    sm.M[(e >> 6) * BW_P + (e & 63)] = L[(int64_t)(BW_TILE * i + (e >> 6)) * B + BW_TILE * i + (e & 63)];
  __syncthreads();
}

// sm.v <- L^-1 sm.v, 64 rows at a time
template <int B>
__device__ void bw_lower(BwSolveLds<B> &sm, const double *L) {
  constexpr int T = B / BW_TILE;
  const int tid = threadIdx.x;
  for (int i = 0; i < T; ++i) {
    if (i > 0) {
      bw_matvec<B>(sm, L + (int64_t)BW_TILE * i * B, B, BW_TILE, BW_TILE * i, sm.v);
      if (tid < BW_TILE) sm.v[BW_TILE * i + tid] -= sm.t[tid];
    }
    bw_stage_tile<B>(sm, L, i);
    if (tid < IPX_WAVE) sm.v[BW_TILE * i + tid] = bt_lower<BW_TILE>(sm.M, sm.v[BW_TILE * i + tid], tid);
  }
  __syncthreads();
}

// sm.v <- L^-T sm.v
template <int B>
__device__ void bw_upper(BwSolveLds<B> &sm, const double *L) {
  constexpr int T = B / BW_TILE;
  const int tid = threadIdx.x;
  for (int i = T - 1; i >= 0; --i) {
    if (i < T - 1) {
      // sum over the rows under tile row i of L[k][64 i + c] x[k]
      bw_tmatvec<B>(sm, L + (int64_t)BW_TILE * (i + 1) * B + BW_TILE * i, B, BW_TILE,
                    B - BW_TILE * (i + 1), sm.v + BW_TILE * (i + 1));
      if (tid < BW_TILE) sm.v[BW_TILE * i + tid] -= sm.t[tid];
    }
    bw_stage_tile<B>(sm, L, i);
    if (tid < IPX_WAVE) sm.v[BW_TILE * i + tid] = bt_upper<BW_TILE>(sm.M, sm.v[BW_TILE * i + tid], tid);
  }
  __syncthreads();
}

// Even row I at stride s (bt_forward): r_I -= V_{I-s}' y_{I-s} + U_{I+s}' y_{I+s}
template <int B>
__global__ void __launch_bounds__(IPX_BLOCK) k_bw_forward(BtStore S, int N, int s) {
  __shared__ BwSolveLds<B> sm;
  const int tid = threadIdx.x;
  const int64_t I = 2 * (int64_t)blockIdx.x * s;
  const bool on = tid < B;
  if (on) sm.acc[tid] = S.r[I * B + tid];
  for (int side = 0; side < 2; ++side) {
    const int64_t J = side ? I + s : I - s;
    if (J < 0 || J >= N) continue;
    __syncthreads();
    if (on) sm.v[tid] = S.r[J * B + tid];
    __syncthreads();
    bw_lower<B>(sm, S.D + J * B * B);
    if (side && on) S.y[J * B + tid] = sm.v[tid];
    bw_tmatvec<B>(sm, (side ? S.E : S.V) + J * B * B, B, B, B, sm.v);
    if (on) sm.acc[tid] -= sm.t[tid];
  }
  if (on) S.r[I * B + tid] = sm.acc[tid];
}

// Odd row J at stride s (bt_back): x_J = L_J^-T (y_J - U_J x_{J-s} - V_J x_{J+s})
template <int B>
__global__ void __launch_bounds__(IPX_BLOCK)
k_bw_back(BtStore S, int N, int s, double *x, int m) {
  __shared__ BwSolveLds<B> sm;
  const int tid = threadIdx.x;
  const int64_t J = (2 * (int64_t)blockIdx.x + 1) * s;
  const bool on = tid < B;
  if (on) sm.acc[tid] = S.y[J * B + tid];
  for (int side = 0; side < 2; ++side) {
    const int64_t I = side ? J + s : J - s;
    if (I < 0 || I >= N) continue;
    __syncthreads();
    if (on) sm.v[tid] = I * B + tid < m ? x[I * B + tid] : 0.0;
    bw_matvec<B>(sm, (side ? S.V : S.E) + J * B * B, B, B, B, sm.v);
    if (on) sm.acc[tid] -= sm.t[tid];
  }
  __syncthreads();
  if (on) sm.v[tid] = sm.acc[tid];
  __syncthreads();
  bw_upper<B>(sm, S.D + J * B * B);
  if (on && J * B + tid < m) x[J * B + tid] = sm.v[tid];
}

// The last block (row 0): x_0 = L_0^-T L_0^-1 r_0
template <int B>
__global__ void __launch_bounds__(IPX_BLOCK) k_bw_top(BtStore S, double *x, int m) {
  __shared__ BwSolveLds<B> sm;
  const int tid = threadIdx.x;
  if (tid < B) sm.v[tid] = S.r[tid];
  __syncthreads();
  bw_lower<B>(sm, S.D);
  bw_upper<B>(sm, S.D);
  if (tid < B && tid < m) x[tid] = sm.v[tid];
}

template <int B>
int bw_solve(int64_t m, int64_t N, double *ws, const double *w, double *x, hipStream_t st) {
  const BtStore S = bt_store(ws, N, B);
  hipLaunchKernelGGL(k_bt_rhs, dim3((unsigned)((N * B + IPX_BLOCK - 1) / IPX_BLOCK)),
                     dim3(IPX_BLOCK), 0, st, N * B, (int)m, w, S.r);
  IPX_CHECK_LAUNCH();
  int s = 1, n = (int)N;
  while (n > 1) {
    hipLaunchKernelGGL(k_bw_forward<B>, dim3((n + 1) / 2), dim3(IPX_BLOCK), 0, st, S, (int)N, s);
    IPX_CHECK_LAUNCH();
    s *= 2;
    n = (n + 1) / 2;
  }
  hipLaunchKernelGGL(k_bw_top<B>, dim3(1), dim3(IPX_BLOCK), 0, st, S, x, (int)m);
  IPX_CHECK_LAUNCH();
  while (s > 1) {
    s /= 2;
    n = (int)((N + s - 1) / s);
    hipLaunchKernelGGL(k_bw_back<B>, dim3(n / 2), dim3(IPX_BLOCK), 0, st, S, (int)N, s, x, (int)m);
    IPX_CHECK_LAUNCH();
  }
  return IPX_OK;
}

}  // namespace

extern "C" {

int ipx_blockwide_kmax(void) { return BW_KMAX; }

int64_t ipx_blockwide_ws_doubles(int64_t m, int32_t b) {
  if (m < 1 || !bw_valid_b(b)) return 0;
  const int64_t N = (m + b - 1) / b;
  return 3 * N * b * b + 3 * N * b;
}

int ipx_blockwide_levels(int64_t m, int32_t b, int32_t out[2]) {
  if (m < 1 || !bw_valid_b(b) || !out) return IPX_EINVAL;
  const int64_t N = (m + b - 1) / b;
  int levels = 1;
  for (int64_t n = N; n > 1; n = (n + 1) / 2) ++levels;
  out[0] = levels;
  out[1] = 1;                                         // no one-workgroup tail
  return levels - 1;
}

int ipx_aat_blockwide(int64_t m, int32_t b, int32_t k, const int32_t *rowptr,
                      const int32_t *colidx, const double *val, const int32_t *perm, double *D,
                      double *E, void *stream) {
  if (m < 1 || m > INT32_MAX - BW_KMAX || !bw_valid_b(b) || k < 0 || k > b || !rowptr || !D || !E)
    return IPX_EINVAL;
  const int64_t N = (m + b - 1) / b, tot = 2 * N * b * b;
  hipLaunchKernelGGL(k_bt_aat, dim3((unsigned)((tot + IPX_BLOCK - 1) / IPX_BLOCK)),
                     dim3(IPX_BLOCK), 0, (hipStream_t)stream, (int)m, b, k, N, rowptr, colidx, val,
                     perm, D, E);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

int ipx_blockwide_factor(int64_t m, int32_t b, const double *D, const double *E, double *ws,
                         int *flag, void *stream) {
  if (m < 1 || m > INT32_MAX - BW_KMAX || !bw_valid_b(b) || !D || !E || !ws || !flag)
    return IPX_EINVAL;
  const int64_t N = (m + b - 1) / b;
  hipStream_t st = (hipStream_t)stream;
  if (b == 128) return bw_factor<128>(N, D, E, ws, flag, st);
  return bw_factor<256>(N, D, E, ws, flag, st);
}

int ipx_blockwide_solve(int64_t m, int32_t b, double *ws, const double *w, double *x,
                        void *stream) {
  if (m < 1 || m > INT32_MAX - BW_KMAX || !bw_valid_b(b) || !ws || !w || !x || w == x)
    return IPX_EINVAL;
  const int64_t N = (m + b - 1) / b;
  hipStream_t st = (hipStream_t)stream;
  if (b == 128) return bw_solve<128>(m, N, ws, w, x, st);
  return bw_solve<256>(m, N, ws, w, x, st);
}

int ipx_blocktri_kmax(void) { return BT_KMAX; }

int64_t ipx_blocktri_ws_doubles(int64_t m, int32_t b) {
  if (m < 1 || !bt_valid_b(b)) return 0;
  const int64_t N = (m + b - 1) / b;
  return 3 * N * b * b + 3 * N * b;
}

int ipx_blocktri_levels(int64_t m, int32_t b, int32_t out[2]) {
  if (m < 1 || !bt_valid_b(b) || !out) return IPX_EINVAL;
  const int64_t N = (m + b - 1) / b;
  int levels = 1, launched = 0;
  for (int64_t n = N; n > 1; n = (n + 1) / 2) {
    ++levels;
    if (n > BT_TAIL_ROWS / b) ++launched;
  }
  out[0] = levels;
  out[1] = BT_TAIL_ROWS / b;
  return launched;
}

int ipx_aat_blocktri(int64_t m, int32_t b, int32_t k, const int32_t *rowptr,
                     const int32_t *colidx, const double *val, const int32_t *perm, double *D,
                     double *E, void *stream) {
  if (m < 1 || m > INT32_MAX - 64 || !bt_valid_b(b) || k < 0 || k > b || !rowptr || !D || !E)
    return IPX_EINVAL;
  const int64_t N = (m + b - 1) / b, tot = 2 * N * b * b;
  hipLaunchKernelGGL(k_bt_aat, dim3((unsigned)((tot + IPX_BLOCK - 1) / IPX_BLOCK)),
                     dim3(IPX_BLOCK), 0, (hipStream_t)stream, (int)m, b, k, N, rowptr, colidx, val,
                     perm, D, E);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

int ipx_blocktri_factor(int64_t m, int32_t b, const double *D, const double *E, double *ws,
                        int *flag, void *stream) {
  if (m < 1 || m > INT32_MAX - 64 || !bt_valid_b(b) || !D || !E || !ws || !flag)
    return IPX_EINVAL;
  const int64_t N = (m + b - 1) / b;
  hipStream_t st = (hipStream_t)stream;
  if (b == 16) return bt_factor<16>(N, D, E, ws, flag, st);
  if (b == 32) return bt_factor<32>(N, D, E, ws, flag, st);
  return bt_factor<64>(N, D, E, ws, flag, st);
}

int ipx_blocktri_solve(int64_t m, int32_t b, double *ws, const double *w, double *x,
                       void *stream) {
  if (m < 1 || m > INT32_MAX - 64 || !bt_valid_b(b) || !ws || !w || !x || w == x)
    return IPX_EINVAL;
  const int64_t N = (m + b - 1) / b;
  hipStream_t st = (hipStream_t)stream;
  if (b == 16) return bt_solve<16>(m, N, ws, w, x, st);
  if (b == 32) return bt_solve<32>(m, N, ws, w, x, st);
  return bt_solve<64>(m, N, ws, w, x, st);
}

}  // extern "C"
