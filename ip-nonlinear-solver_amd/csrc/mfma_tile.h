// The 64 x 64 fp64 MFMA tile shared by the dense kernels: csrc/dense.hip (Gram, blocked Cholesky,
// triangular inverse) and csrc/denseqr.hip (blocked Householder QR).  Device helpers only: the
// K-permuted LDS panel layout (gram_slot / gram_stash), the strided operand (Opnd / opnd_fetch),
// the tile product C = P Q' (tile_pqt) and the walk over a tile's accumulators
// (IPX_TILE_FOREACH).  Every kernel keeps its own LDS arrays and its own epilogue.
#pragma once
#include "ipx_common.h"

typedef double v4d __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));

constexpr int GT = 64;          // tile edge of G per workgroup
constexpr int GK = 32;          // K chunk
constexpr int GSP = 10;         // sub-panel row pitch (doubles): 8 k-values of one lane group + 2
constexpr int GSUB = GT * GSP;  // sub-panel (one lane group lk): 640 doubles = 320 slots
constexpr int GPANEL = 4 * GSUB;

// Which double2 of the 64 x 32 panel thread `tid` moves in its u-th load / LDS store: row r,
// column pair t (columns 2t, 2t+1).  A wave instruction covers four whole rows' 256-byte
// chunks (coalesced), and every 8 CONTIGUOUS lanes -- the banking group of ds_write_b128,
// modulo 32 dwords -- write one lane group's (lk) pairs j = 0..3 of rows b and b + 4: dword
// offsets 20 row + 4 j = const + {0, 4, ..., 28}, every bank once.  (idx -> (idx >> 4,
// idx & 15) put the four lk of one row and j on the same banks: 4-way conflicts.)
__device__ __forceinline__ void gram_slot(int tid, int u, int &r, int &t) {
  const int lane = tid & 63, wave = tid >> 6;
  const int c = wave * 4 + u;                    // 16 (wave, u) combinations x 4 rows
  const int b = 8 * (c >> 1) + 2 * (c & 1);      // rows b, b+1, b+4, b+5
  const int g = lane >> 3, i = lane & 7;
  const int j = i & 3, rsel = i >> 2, lk = g & 3, rpair = g >> 2;
  r = b + 4 * rsel + rpair;
  t = 4 * j + lk;
}

__device__ __forceinline__ void gram_stash(double *panel, int tid, const v2d (&reg)[4]) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    int r, t;
    gram_slot(tid, u, r, t);                      // columns 2t, 2t + 1 = 8 j + 2 lk + {0, 1}
    const int j = t >> 2, lk = t & 3;
    *reinterpret_cast<v2d *>(panel + lk * GSUB + r * GSP + 2 * j) = reg[u];
  }
}

// element (i, k) of a 64 x K operand panel at p[i * rs + k * ks]
struct Opnd {
  const double *p;
  int64_t rs, ks;
};

__device__ __forceinline__ void opnd_fetch(const Opnd &O, int k0, int tid, v2d (&reg)[4]) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    int r, t;
    gram_slot(tid, u, r, t);
    const double *src = O.p + (int64_t)r * O.rs + (int64_t)(k0 + 2 * t) * O.ks;
    reg[u] = (v2d){src[0], src[O.ks]};
  }
}

// acc (the 64 x 64 tile C = P Q', summed over k in [0, K), K a multiple of 32) by the four
// waves of the workgroup: element (row, col) = (wr + 16 a + lk + 4 reg, wc + 16 b + lr) in
// acc[a][b][reg] (k_gram_mfma's layout).  sA / sB: GPANEL doubles each.
__device__ __forceinline__ void tile_pqt(const Opnd &P, const Opnd &Q, int K, v4d (&acc)[2][2],
                                         double *sA, double *sB) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
  const int lr = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (v4d){0.0, 0.0, 0.0, 0.0};
  if (K <= 0) return;
  v2d ra[4], rb[4];
  opnd_fetch(P, 0, tid, ra);
  opnd_fetch(Q, 0, tid, rb);
  for (int k0 = 0; k0 < K; k0 += GK) {
    gram_stash(sA, tid, ra);
    gram_stash(sB, tid, rb);
    __syncthreads();
    if (k0 + GK < K) {
      opnd_fetch(P, k0 + GK, tid, ra);
      opnd_fetch(Q, k0 + GK, tid, rb);
    }
    const double *qa = sA + lk * GSUB + (wr + lr) * GSP;
    const double *qb = sB + lk * GSUB + (wc + lr) * GSP;
#pragma unroll
    for (int j = 0; j < GK / 8; ++j) {
      const v2d a0 = *reinterpret_cast<const v2d *>(qa + 2 * j);
      const v2d a1 = *reinterpret_cast<const v2d *>(qa + 16 * GSP + 2 * j);
      const v2d b0 = *reinterpret_cast<const v2d *>(qb + 2 * j);
      const v2d b1 = *reinterpret_cast<const v2d *>(qb + 16 * GSP + 2 * j);
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.x, b0.x, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.x, b1.x, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.x, b0.x, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.x, b1.x, acc[1][1], 0, 0, 0);
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.y, b0.y, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.y, b1.y, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.y, b0.y, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.y, b1.y, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
}

// for (row, col, value) of the tile held in acc
#define IPX_TILE_FOREACH(acc, row, col, val, ...)                                    \
  do {                                                                                \
    const int lane_ = threadIdx.x & 63, wave_ = threadIdx.x >> 6;                     \
    const int wr_ = (wave_ >> 1) * 32, wc_ = (wave_ & 1) * 32;                        \
    const int lr_ = lane_ & 15, lk_ = lane_ >> 4;                                     \
    _Pragma("unroll") for (int a_ = 0; a_ < 2; ++a_)                                  \
    _Pragma("unroll") for (int b_ = 0; b_ < 2; ++b_)                                  \
    _Pragma("unroll") for (int g_ = 0; g_ < 4; ++g_) {                                \
      const int row = wr_ + 16 * a_ + lk_ + 4 * g_, col = wc_ + 16 * b_ + lr_;        \
      const double val = acc[a_][b_][g_];                                             \
      __VA_ARGS__;                                                                    \
    }                                                                                 \
  } while (0)
