// What the Householder QR kernels of csrc/denseqr.hip (unpivoted, k_qr_panel) and
// csrc/denseqrp.hip (column-pivoted, k_qrp_select / k_qrp_reflect) share, so that the two
// factorizations agree by construction: the chunk geometry of a row of W, the reflector of one
// step (dlarfg) and the guarded loads / stores of a row's chunk.
#pragma once
#include <limits.h>

#include "ipx_common.h"

// A workgroup works on a chunk of 512 consecutive columns of the rows of W (M x N): lane l of
// every wave holds the columns kbase + 64 u, u < QR_U, kbase = 512 chunk + l.
constexpr int QR_CHUNK = 512;
constexpr int QR_U = QR_CHUNK / IPX_WAVE;

static inline int qr_chunks(int64_t N) { return (int)((N + QR_CHUNK - 1) / QR_CHUNK); }

// grid of an element-wise kernel: one thread per element
static inline unsigned qr_grid(int64_t elements) {
  return (unsigned)ipx_grid_for(elements, IPX_BLOCK, INT_MAX);
}

// The reflector H = I - tau v v', v = (1, x * inv), that takes (alpha, x) to (beta, 0), from
// alpha and tail2 = ||x||^2 (dlarfg).  A zero tail: H = I, tau = 0, beta = alpha.
struct QrReflector {
  double beta, tau, inv;
};
__device__ __forceinline__ QrReflector qr_dlarfg(double alpha, double tail2) {
  QrReflector h{alpha, 0.0, 0.0};
  if (tail2 != 0.0) {
    h.beta = -copysign(sqrt(alpha * alpha + tail2), alpha);
    h.tau = (h.beta - alpha) / h.beta;
    h.inv = 1.0 / (alpha - h.beta);
  }
  return h;
}

// x[u] <- row[k] for this lane's columns k < N of the chunk, 0 from column N on
__device__ __forceinline__ void qr_load_chunk(const double *row, int kbase, int N,
                                              double (&x)[QR_U]) {
#pragma unroll
  for (int u = 0; u < QR_U; ++u) {
    const int k = kbase + u * IPX_WAVE;
    x[u] = k < N ? row[k] : 0.0;
  }
}

// row[k] <- x[u] for this lane's columns k of the chunk with lo <= k < N
__device__ __forceinline__ void qr_store_chunk(double *row, int kbase, int lo, int N,
                                               const double (&x)[QR_U]) {
#pragma unroll
  for (int u = 0; u < QR_U; ++u) {
    const int k = kbase + u * IPX_WAVE;
    if (k < N && k >= lo) row[k] = x[u];
  }
}

// v <- reflector j on this chunk from the row that holds its unscaled tail: (0 .. 0, 1 at
// column j, row[k] * inv for k > j), 0 from column N on
__device__ __forceinline__ void qr_reflector_chunk(const double *row, int kbase, int j,
                                                   int N, double inv, double (&v)[QR_U]) {
#pragma unroll
  for (int u = 0; u < QR_U; ++u) {
    const int k = kbase + u * IPX_WAVE;
    v[u] = 0.0;
    if (k < N) v[u] = k > j ? row[k] * inv : (k == j ? 1.0 : 0.0);
  }
}
