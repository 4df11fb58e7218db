// Dense constraint Jacobians with inequality rows (device-callback mode; the reference's dense
// canonical form _canonical_constraint.py:240-280, :363-438 and the barrier's augmented
// Jacobian tr_interior_point.py:141-194).  Pure data movement, no arithmetic beyond a sign and
// the slack squares: every kernel here is HBM-bound.
//
//   ipx_dense_gather_rows   out[dst[r], col0 + j] = sign[r] * src[idx[r], j]   (row selection,
//                           re-signing and stacking of several parts into one buffer)
//   ipx_csr_rows_to_dense   the same for the rows of a CSR part (a sparse or box constraint
//                           stacked next to a dense one: canonical._stack_dense)
//   ipx_dense_augment       A = [[J_eq, 0], [J_ineq, diag(s)]] and, in the same pass, A'
//   ipx_gram_shift          G = G0 + diag(0_{m_eq}, s*s) on the padded M x M Gram layout (s
//                           strided: read straight off the diagonal block of the augmented A)
#include "ipx_common.h"

namespace {

// One workgroup per destination row.  16-byte accesses along the row where source and
// destination rows share their 16-byte phase (one element peeled at the front when both start
// on an odd double); 8-byte accesses otherwise (odd leading dimensions).
__global__ void __launch_bounds__(IPX_BLOCK)
k_gather_rows(int64_t ncols, const double *__restrict__ src, int64_t lds,
              const int32_t *__restrict__ idx, const double *__restrict__ sign,
              const int32_t *__restrict__ dst, double *__restrict__ out, int64_t ldo,
              int64_t col0) {
  const int64_t r = blockIdx.x;
  const int64_t sr = idx ? (int64_t)idx[r] : r;
  const int64_t dr = dst ? (int64_t)dst[r] : r;
  const double g = sign ? sign[r] : 1.0;
  const double *s = src + sr * lds;
  double *o = out + dr * ldo + col0;
  const int sa = (int)(((uintptr_t)s >> 3) & 1), oa = (int)(((uintptr_t)o >> 3) & 1);
  if (sa == oa && ((uintptr_t)s & 7) == 0 && ((uintptr_t)o & 7) == 0) {
    int64_t head = 0;
    if (sa && ncols > 0) {
      if (threadIdx.x == 0) o[0] = g * s[0];
      head = 1;
    }
    const int64_t n2 = (ncols - head) >> 1;
    const double2 *s2 = reinterpret_cast<const double2 *>(s + head);
    double2 *o2 = reinterpret_cast<double2 *>(o + head);
    for (int64_t j = threadIdx.x; j < n2; j += IPX_BLOCK) {
      double2 v = s2[j];
      v.x = g * v.x;
      v.y = g * v.y;
      o2[j] = v;
    }
    const int64_t tail = head + 2 * n2;
    if (tail < ncols && threadIdx.x == 0) o[tail] = g * s[tail];
  } else {
    for (int64_t j = threadIdx.x; j < ncols; j += IPX_BLOCK) o[j] = g * s[j];
  }
}

// One workgroup per destination row: the row is zeroed by the workgroup, then lane 0 adds the
// row's nonzeros in storage order (duplicate column entries are summed like scipy's toarray;
// no two lanes ever write one address).
__global__ void __launch_bounds__(IPX_BLOCK)
k_csr_rows_to_dense(int64_t ncols, const int32_t *__restrict__ rowptr,
                    const int32_t *__restrict__ colidx, const double *__restrict__ val,
                    const int32_t *__restrict__ idx, const double *__restrict__ sign,
                    const int32_t *__restrict__ dst, double *__restrict__ out, int64_t ldo) {
  const int64_t r = blockIdx.x;
  const int64_t sr = idx ? (int64_t)idx[r] : r;
  const int64_t dr = dst ? (int64_t)dst[r] : r;
  double *o = out + dr * ldo;
  for (int64_t j = threadIdx.x; j < ncols; j += IPX_BLOCK) o[j] = 0.0;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double g = sign ? sign[r] : 1.0;
    const int32_t kb = rowptr[sr], ke = rowptr[sr + 1];
    for (int32_t k = kb; k < ke; ++k) {
      const int32_t c = colidx[k];
      if (c >= 0 && c < ncols) o[c] = o[c] + g * val[k];
    }
  }
}

// A tile of AUG_R rows x AUG_C columns of A per workgroup: each wave writes whole 64-column
// segments of A's rows (512 B contiguous), the tile goes through LDS (rows padded by one
// double: the column reads of a half-wave hit 32 distinct bank pairs) and comes out as AUG_C
// rows x AUG_R columns of A' (half-waves write 256 B contiguous).
constexpr int AUG_R = 32, AUG_C = 64;

template <bool TRANSPOSE>
__global__ void __launch_bounds__(IPX_BLOCK)
k_dense_augment(int64_t m_eq, int64_t m_in, int64_t n, const double *__restrict__ J_eq,
                int64_t ld_eq, const double *__restrict__ J_in, int64_t ld_in,
                const double *__restrict__ s, double *__restrict__ A,
                double *__restrict__ At) {
  __shared__ double tile[AUG_R][AUG_C + 1];
  const int64_t m = m_eq + m_in, N = n + m_in;
  const int64_t i0 = (int64_t)blockIdx.y * AUG_R, j0 = (int64_t)blockIdx.x * AUG_C;
  const int lane = threadIdx.x & (AUG_C - 1), wrow = threadIdx.x / AUG_C;
  const int64_t j = j0 + lane;
#pragma unroll
  for (int p = 0; p < AUG_R / (IPX_BLOCK / AUG_C); ++p) {
    const int rr = p * (IPX_BLOCK / AUG_C) + wrow;
    const int64_t i = i0 + rr;
    double v = 0.0;
    if (i < m && j < N) {
      if (i < m_eq) {
        if (j < n) v = J_eq[i * ld_eq + j];
      } else {
        const int64_t k = i - m_eq;
        if (j < n) v = J_in[k * ld_in + j];
        else if (j - n == k) v = s[k];
      }
      if (A) A[i * N + j] = v;
    }
    if (TRANSPOSE) tile[rr][lane] = v;
  }
  if (!TRANSPOSE) return;
  __syncthreads();
  const int col = threadIdx.x & (AUG_R - 1), trow = threadIdx.x / AUG_R;
  const int64_t i = i0 + col;
#pragma unroll
  for (int p = 0; p < AUG_C / (IPX_BLOCK / AUG_R); ++p) {
    const int cc = p * (IPX_BLOCK / AUG_R) + trow;
    const int64_t jj = j0 + cc;
    if (jj < N && i < m) At[jj * m + i] = tile[col][cc];
  }
}

// G = G0 + diag(0, s*s): one workgroup per row of the padded M x M layout, 16-byte copies (M is
// a multiple of 64), the diagonal entry of rows m_eq..m-1 shifted by the thread that copies it.
__global__ void __launch_bounds__(IPX_BLOCK)
k_gram_shift_copy(int64_t M, int64_t m_eq, int64_t m, const double *__restrict__ G0,
                  const double *__restrict__ s, int64_t incs, double *__restrict__ G) {
  const int64_t row = blockIdx.x;
  const double2 *src = reinterpret_cast<const double2 *>(G0 + row * M);
  double2 *dst = reinterpret_cast<double2 *>(G + row * M);
  const bool shifted = row >= m_eq && row < m;
  const double sk = shifted ? s[(row - m_eq) * incs] : 0.0;
  const double sq = sk * sk;
  for (int64_t q = threadIdx.x; q < M / 2; q += IPX_BLOCK) {
    double2 v = src[q];
    if (shifted) {
      if (2 * q == row) v.x = v.x + sq;
      else if (2 * q + 1 == row) v.y = v.y + sq;
    }
    dst[q] = v;
  }
}

// In place: G[i, i] += s[(i - m_eq) * incs]^2 for m_eq <= i < m.
__global__ void __launch_bounds__(IPX_BLOCK)
k_gram_shift_diag(int64_t M, int64_t m_eq, int64_t m_in, const double *__restrict__ s,
                  int64_t incs, double *__restrict__ G) {
  const int64_t k = (int64_t)blockIdx.x * IPX_BLOCK + threadIdx.x;
  if (k >= m_in) return;
  const double sk = s[k * incs];
  const double sq = sk * sk;
  const int64_t i = m_eq + k;
  G[i * M + i] = G[i * M + i] + sq;
}

}  // namespace

extern "C" {

int ipx_dense_gather_rows(int64_t rows, int64_t ncols, const double *src, int64_t lds,
                          const int32_t *idx, const double *sign, const int32_t *dst,
                          double *out, int64_t ldo, int64_t col0, void *stream) {
  if (rows < 0 || ncols < 0 || col0 < 0) return IPX_EINVAL;
  if (rows == 0 || ncols == 0) return IPX_OK;
  if (!src || !out || lds < ncols || ldo < col0 + ncols || rows > INT32_MAX) return IPX_EINVAL;
  hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)rows), dim3(IPX_BLOCK), 0,
                     (hipStream_t)stream, ncols, src, lds, idx, sign, dst, out, ldo, col0);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

int ipx_csr_rows_to_dense(int64_t rows, int64_t ncols, const int32_t *rowptr,
                          const int32_t *colidx, const double *val, const int32_t *idx,
                          const double *sign, const int32_t *dst, double *out, int64_t ldo,
                          void *stream) {
  if (rows < 0 || ncols < 0) return IPX_EINVAL;
  if (rows == 0 || ncols == 0) return IPX_OK;
  if (!rowptr || !out || ldo < ncols || rows > INT32_MAX) return IPX_EINVAL;
  hipLaunchKernelGGL(k_csr_rows_to_dense, dim3((unsigned)rows), dim3(IPX_BLOCK), 0,
                     (hipStream_t)stream, ncols, rowptr, colidx, val, idx, sign, dst, out, ldo);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

int ipx_dense_augment(int64_t m_eq, int64_t m_in, int64_t n, const double *J_eq, int64_t ld_eq,
                      const double *J_in, int64_t ld_in, const double *s, double *A, double *At,
                      void *stream) {
  if (m_eq < 0 || m_in < 0 || n < 0 || (!A && !At)) return IPX_EINVAL;
  if ((m_eq > 0 && n > 0 && (!J_eq || ld_eq < n)) || (m_in > 0 && (!s || (n > 0 && (!J_in ||
      ld_in < n)))))
    return IPX_EINVAL;
  const int64_t m = m_eq + m_in, N = n + m_in;
  if (m == 0 || N == 0) return IPX_OK;
  const int64_t gx = (N + AUG_C - 1) / AUG_C, gy = (m + AUG_R - 1) / AUG_R;
  if (gx > INT32_MAX || gy > 65535) return IPX_EINVAL;
  const dim3 grid((unsigned)gx, (unsigned)gy);
  if (At)
    hipLaunchKernelGGL(k_dense_augment<true>, grid, dim3(IPX_BLOCK), 0, (hipStream_t)stream,
                       m_eq, m_in, n, J_eq, ld_eq, J_in, ld_in, s, A, At);
  else
    hipLaunchKernelGGL(k_dense_augment<false>, grid, dim3(IPX_BLOCK), 0, (hipStream_t)stream,
                       m_eq, m_in, n, J_eq, ld_eq, J_in, ld_in, s, A, At);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

int ipx_gram_shift(int64_t m, int64_t m_eq, const double *G0, const double *s, int64_t incs,
                   double *G, void *stream) {
  if (m < 1 || m_eq < 0 || m_eq > m || !G || (m_eq < m && (!s || incs < 1))) return IPX_EINVAL;
  const int64_t M = ipx_dense_padded(m), m_in = m - m_eq;
  if (G0) {
    if (((uintptr_t)G0 | (uintptr_t)G) % 16) return IPX_EINVAL;
    hipLaunchKernelGGL(k_gram_shift_copy, dim3((unsigned)M), dim3(IPX_BLOCK), 0,
                       (hipStream_t)stream, M, m_eq, m, G0, s, incs, G);
    IPX_CHECK_LAUNCH();
  } else if (m_in > 0) {
    hipLaunchKernelGGL(k_gram_shift_diag, dim3((unsigned)((m_in + IPX_BLOCK - 1) / IPX_BLOCK)),
                       dim3(IPX_BLOCK), 0, (hipStream_t)stream, M, m_eq, m_in, s, incs, G);
    IPX_CHECK_LAUNCH();
  }
  return IPX_OK;
}

}  // extern "C"
