/*
 * ipx.h -- C ABI of the MI355X-native trust-region subproblem kernels.
 *
 * Drop-in boundary for the hot path of antonior92/ip-nonlinear-solver
 * (SURVEY.md section 8(b)).  The reference is pure Python: its "FFI" for this
 * path is the duck-typed operator seam
 *
 *     H.dot(v), A.dot(v), A.T.dot(v)        qp_subproblem.py:376,379,410,503,634
 *     Z.dot(v), LS.dot(v), Y.dot(v)         projections.py:402-404
 *     np.dot / norm / elementwise algebra   qp_subproblem.py:99-232,502-634
 *
 * so the entry points below are what a ctypes binding of that seam binds
 * (INTEGRATION.md shows the stub).  Conventions:
 *   - every pointer is a DEVICE pointer owned by the caller (the Python host
 *     keeps them alive as torch tensors); the library allocates nothing the
 *     caller can see except opaque handles with an explicit *_destroy;
 *   - every call takes the hipStream_t to enqueue on (as void*), never
 *     synchronises the device, and returns 0 or a negative IPX_E* code;
 *   - fp64 values, int32 indices (scipy's defaults);
 *   - reductions are two-stage and fixed-order: stage 1 writes one partial
 *     per workgroup into a caller workspace, stage 2 sums them in index
 *     order, so results do not depend on scheduling.
 */
#ifndef IPX_H
#define IPX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IPX_OK 0
#define IPX_EINVAL (-1)    /* bad argument */
#define IPX_ELAUNCH (-2)   /* HIP launch / runtime error */
#define IPX_ENOTSPD (-3)   /* factorization met a non-positive pivot */
#define IPX_ENOMEM (-4)
#define IPX_EUNSUPPORTED (-5) /* this solver has no path for the matrix at hand: take another */
#define IPX_EILLCOND (-6)  /* ipx_banded_status: factorization complete, but a pivot lost 43 bits
                            * against its diagonal entry (numerically rank-deficient Jacobian) */

/* Number of doubles of reduction workspace any entry point may need. */
#define IPX_WS_DOUBLES 65536
/* Max partials a fused kernel writes per reduced quantity. */
#define IPX_MAX_PARTIALS 2048

const char *ipx_version(void);
/* Kernel launches of the library since it was loaded (a host counter: diagnostics, bench.py). */
long long ipx_launch_count(void);
/* Blocking reads of the library since it was loaded: every wait for device results -- ipx_read_doubles
 * / ipx_read_folded, and the chains of csrc/sqp.hip that hand over their block themselves. */
long long ipx_read_count(void);
/* Text of the last HIP error seen by this thread ("" if none). */
const char *ipx_last_error(void);
int ipx_device_info(int *cu_count, int *lds_bytes, char *arch, int arch_len);
/* Blocking read-back of k <= 512 doubles of device memory behind everything queued on `stream`
 * (pinned staging buffer inside the library; host_out: k doubles of the caller's). */
int ipx_read_doubles(const double *dev, int k, double *host_out, void *stream);
/* ... of nd <= IPX_FOLD_MAX scalars, each folded from a partial array (op: 0 sum, 1 max, 2 min) */
#define IPX_FOLD_MAX 32
typedef struct {
  const double *part;
  int32_t count;
  int32_t op;
} ipx_fold_desc;
int ipx_read_folded(int nd, const ipx_fold_desc *descs, double *host_out, void *stream);
/* ... and their weighted sum left on the device instead (no read): out[0] = ((w[0] r_0 + w[1] r_1)
 * + w[2] r_2) + ... -- an objective value assembled from dot products that only a later kernel
 * consumes (ipx_sqp_judge's f_next_dev; ipsolver.device.ScalarPack.combine). */
int ipx_fold_combine(int nd, const ipx_fold_desc *descs, const double *weights, double *out,
                     void *stream);

/* ---- vectors (np elementwise algebra; qp_subproblem.py:212-216,312,580,622,628)
 * out = a*x + b*y (y may be NULL when b == 0); in-place allowed. */
int ipx_axpby(int64_t n, double a, const double *x, double b, const double *y,
              double *out, void *stream);
/* out = x * y elementwise (diagonal scaling S.dot(d), tr_interior_point.py:111) */
int ipx_mul(int64_t n, const double *x, const double *y, double *out, void *stream);
int ipx_fill(int64_t n, double value, double *out, void *stream);
/* out = min(max(x, lb), ub): reinforce_box_boundaries, qp_subproblem.py:310-317 */
int ipx_clip(int64_t n, const double *x, const double *lb, const double *ub,
             double *out, void *stream);
/* out[i] = a*x[i] + b (scalar shift) */
int ipx_affine(int64_t n, double a, const double *x, double b, double *out, void *stream);

/* out[i] = sign[i] * (x[idx[i]] - shift[i]); sign / shift may be NULL.  Row
 * selection + sign flip of the canonical constraint form
 * (_canonical_constraint.py:240-248) and permutation of constraint-space vectors. */
int ipx_gather(int64_t n, const double *x, const int32_t *idx, const double *sign,
               const double *shift, double *out, void *stream);

/* out[idx[i]] = x[i] (refresh of the slack entries of the augmented Jacobian,
 * tr_interior_point.py:186-191). */
int ipx_scatter(int64_t n, const double *x, const int32_t *idx, double *out, void *stream);
/* out[idx[i]] += x[i], idx without repeats (no atomics). */
int ipx_scatter_add(int64_t n, const double *x, const int32_t *idx, double *out, void *stream);
/* Barrier elementwise ops (tr_interior_point.py:92-93,216-220,294):
 * out = max(x, c);  out = v > 0 ? a : c;  s[mask != 0] = -c[mask != 0]. */
int ipx_max_scalar(int64_t n, const double *x, double c, double *out, void *stream);
int ipx_where_positive(int64_t n, const double *v, const double *a, double c, double *out,
                       void *stream);
int ipx_assign_negated_where(int64_t n, double *s, const double *mask, const double *c,
                             void *stream);
/* out[0] = sum log(s_i) over s_i > 0, out[1] = #{s_i <= 0} (the reference's
 * log-barrier term is -inf when out[1] > 0). */
int ipx_sum_log(int64_t n, const double *s, double *out, double *ws, void *stream);

/* ---- reductions.  `out` is a device array; `ws` >= IPX_WS_DOUBLES doubles.
 * ipx_dot:      out[0] = sum x*y                      (np.dot)
 * ipx_norms:    out[0] = sum x^2, out[1] = max |x|    (norm(.), norm(., inf))
 * ipx_box_inside: out[0] = #{i: x<lb or x>ub}         (inside_box_boundaries :306-308)
 * ipx_box_sphere_reduce (box_intersections :198-216 + sphere_intersections :112-114):
 *   out[0]=d.d out[1]=z.d out[2]=z.z
 *   out[3]=max_i min(t_lb,t_ub) out[4]=min_i max(t_lb,t_ub) over d_i != 0
 *   out[5]=#{i: d_i==0 and (z_i<lb_i or z_i>ub_i)}   out[6]=#{i: d_i != 0}
 *   with z' = z0 + zs*z? no: z is used as given; d is scaled by `dscale`
 *   (the reference passes alpha*p, :585). lb/ub may be NULL (= -inf/+inf). */
int ipx_dot(int64_t n, const double *x, const double *y, double *out,
            double *ws, void *stream);
int ipx_norms(int64_t n, const double *x, double *out, double *ws, void *stream);
/* The first stage of ipx_dot / ipx_norms alone: ipx_reduce_grid(n) partials per quantity at
 * part[q * grid + workgroup] (norms: q = 0 the sum of squares, q = 1 max |x|), for results only
 * the host wants -- ipx_read_folded folds them inside the read-back, in the order of the
 * second launch of ipx_dot / ipx_norms (same bits), so such a reduction is ONE launch. */
int ipx_reduce_grid(int64_t n);
int ipx_dot_partials(int64_t n, const double *x, const double *y, double *part, void *stream);
int ipx_norms_partials(int64_t n, const double *x, double *part, void *stream);
int ipx_box_inside(int64_t n, const double *x, const double *lb, const double *ub,
                   double *out, double *ws, void *stream);
int ipx_box_sphere_reduce(int64_t n, const double *z, const double *d, double dscale,
                          const double *lb, const double *ub, double *out,
                          double *ws, void *stream);

/* ---- CSR SpMV (scipy _sparsetools csr_matvec; every A.dot / A.T.dot / H.dot).
 * Row tiles: `tiles` holds 2*(ntiles+1) entries -- ntiles+1 row indices (tile t
 * = rows [tiles[t], tiles[t+1])) followed by rowptr at those rows -- with at
 * most IPX_SPMV_TILE_NNZ nonzeros per tile unless a single row is longer;
 * build it with ipx_csr_tiles_host (cap >= 2*(nrows+2) always suffices).
 *
 * y_out = alpha * (A x)_i  [+ diag_i * x_i]  [+ beta * yin_i]
 * and, when red != NULL, red[0] = sum_i y_out_i^2, red[1] = sum_i xrow_i * y_out_i
 * (xrow = x when the matrix is square, used for p'Hp; pass square=0 otherwise).
 */
#define IPX_FOLD_WS_DOUBLES 16384
#define IPX_SPMV_TILE_NNZ 2048
#define IPX_SPMV_TILE_ROWS 1024   /* max rows per tile the fast path takes */
int ipx_csr_tiles_host(int64_t nrows, const int32_t *rowptr_host, int32_t tile_nnz,
                       int32_t max_rows, int32_t *tiles_out, int64_t cap);
int ipx_csr_spmv(int64_t nrows, int64_t ncols, const int32_t *rowptr,
                 const int32_t *colidx, const double *val,
                 const int32_t *tiles, int32_t ntiles,
                 const double *x, double alpha,
                 const double *diag, double beta, const double *yin,
                 double *yout, int square, double *red, double *ws, void *stream);

/* Extended SpMV for the row-sharded CG: explicit row vector (x may carry halo
 * entries), device stop flag, unfolded per-tile partials; and the fold. */
int ipx_csr_spmv_ex(int64_t nrows, int64_t ncols, const int32_t *rowptr, const int32_t *colidx,
                    const double *val, const int32_t *tiles, int32_t ntiles, const double *x,
                    double alpha, const double *diag, double beta, const double *yin,
                    double *yout, const double *xrow, double *partial, const double *guard,
                    void *stream);
int ipx_fold2(const double *partial, int32_t count, double *red, const double *guard,
              void *stream);

/* ---- dense Jacobian path (projections.py:175-233 QR; here Gram + Cholesky).
 * A is row-major with leading dimension lda.  ipx_dense_gemv mirrors
 * ipx_csr_spmv's fused epilogue (diag only for m == n, IPX_EINVAL otherwise: diag_r pairs
 * with x_r).  G / X are M x M, M = ipx_dense_padded(m). */
int ipx_dense_gemv(int64_t m, int64_t n, const double *A, int64_t lda, const double *x,
                   double alpha, const double *diag, double beta, const double *yin,
                   double *yout, double *red, double *ws, void *stream);
/* y (n) = B' x for a row-major B (m x n, leading dimension ldb), summed in a fixed order. */
int ipx_dense_gemvt(int64_t m, int64_t n, const double *B, int64_t ldb, const double *x, double *y,
                    void *stream);
int64_t ipx_dense_padded(int64_t m);
int ipx_gram_f64_mfma(int64_t m, int64_t n, const double *A, int64_t lda, double *G,
                      void *stream);
/* The same with the sum over the columns cut into `splits` parts (ipx_gram_splits picks the
 * count that evens the tiles out over the CUs; partial tiles in ws, ipx_gram_ws_doubles(m,
 * splits) doubles, added in a fixed order: deterministic). */
int ipx_gram_splits(int64_t m, int64_t n);
int64_t ipx_gram_ws_doubles(int64_t m, int32_t splits);
int ipx_gram_f64_mfma_split(int64_t m, int64_t n, const double *A, int64_t lda, double *G,
                            double *ws, int32_t splits, void *stream);
/* Same G from a CSR A (sparse Jacobian whose A A' is not narrow-banded). */
int ipx_aat_dense(int64_t m, const int32_t *rowptr, const int32_t *colidx, const double *val,
                  double *G, void *stream);
/* Blocked Cholesky G = L L' in place (64 x 64 tiles, the trailing updates on the fp64 matrix
 * cores) and X = G^-1 from it (in-place triangular inverse by recursive doubling in G's
 * storage -- G is consumed --, then X = L^-T L^-1 as MFMA tiles): what a dense NONLINEAR
 * constraint pays per accepted step (reference: a pivoted QR, projections.py:175-233).
 * M = ipx_dense_padded(m), a multiple of 64.
 * work: M + 1 doubles; work[M] <- min pivot / original diagonal (~1/cond(G)). */
int ipx_chol_factor(int64_t M, double *G, int *flag, double *work, void *stream);
int ipx_chol_inverse(int64_t M, double *G, double *X, void *stream);
/* The triangular half of ipx_chol_inverse alone: the lower triangle of G (lower triangular L,
 * the strict upper triangle of its diagonal tiles zero) <- L^-1 in place; the upper triangle
 * outside the diagonal tiles is used as scratch. */
int ipx_trtri_lower(int64_t M, double *G, void *stream);

/* ---- blocked Householder QR of A' for a dense row-major A, m <= n (csrc/denseqr.hip; the
 * reference's dense factorization, projections.py:175-233, unpivoted).  M = ipx_dense_padded(m),
 * N = ipx_qr_padded_cols(n).  ipx_qr_factor: W (M x N) <- the reflectors (row j = v_j with its
 * unit entry), L (M x M) <- R' (lower triangular, identity on the padding), T (M / 64 tiles of
 * 64 x 64) <- the compact WY factors, tau (M), info[0] <- min_j |R_jj| / ||row j of A||,
 * info[1 .. M] <- the squared row norms of A.  ipx_qr_form_q: QT (M x N) <- Q' (row r = column r
 * of Q).  ws: ipx_qr_ws_doubles(m, n) doubles for both.  Plain launches only, every sum in a
 * fixed order. */
int64_t ipx_qr_padded_cols(int64_t n);
int64_t ipx_qr_ws_doubles(int64_t m, int64_t n);
int ipx_qr_factor(int64_t m, int64_t n, const double *A, int64_t lda, double *W, double *L,
                  double *T, double *tau, double *info, double *ws, void *stream);
int ipx_qr_form_q(int64_t m, int64_t n, const double *W, const double *T, double *QT, double *ws,
                  void *stream);
/* T (M / 64 tiles) <- the compact WY factors of reflectors W (M x N, ipx_qr_factor's form) and
 * tau (M) that another factorization made (ipx_qrp_reflectors); ws as for ipx_qr_factor. */
int ipx_qr_wy(int64_t m, int64_t n, const double *W, const double *tau, double *T, double *ws,
              void *stream);
/* Linv (M x M) <- L^-1 = R^-T, strict upper triangle exactly zero; L is kept. */
int ipx_qr_tri_inverse(int64_t M, const double *L, double *Linv, void *stream);

/* ---- column-pivoted Householder QR of A' for a dense row-major A, m <= n (csrc/denseqrp.hip):
 * A' P = Q [R11 R12], the rank r = the number of leading j with |R_jj| > 2^-43 |R_00|.  No row
 * of W (M x N) is moved: iw (ipx_qrp_info_ints(m) ints) = perm (M; perm[j] = the row that is
 * pivot j, a permutation of 0 .. m - 1 on return) | pos (M) | done, rank; dw
 * (ipx_qrp_info_doubles(m) doubles) = tau (M) | diag R (M) | the reflectors' scale factors (M) |
 * the pivot norms of the steps taken, the rejected one included.  ipx_qrp_factor: 2 m + 3 plain
 * launches enqueued at once, every sum in a fixed order; ws: ipx_qrp_ws_doubles(m, n) doubles.
 * ipx_qrp_reflectors: Vp (Mr x N, Mr = ipx_dense_padded(r)), taup (Mr) <- the first r reflectors
 * in pivot order, as ipx_qr_wy / ipx_qr_form_q take them.  ipx_qrp_write_t: T (r x m, leading
 * dimension ldt) <- [R11 R12], exactly zero below the diagonal.  ipx_qrp_fold_columns:
 * out[row][perm[c]] <- in[row][c], c < m. */
int64_t ipx_qrp_ws_doubles(int64_t m, int64_t n);
int64_t ipx_qrp_info_doubles(int64_t m);
int64_t ipx_qrp_info_ints(int64_t m);
int ipx_qrp_factor(int64_t m, int64_t n, const double *A, int64_t lda, double *W, double *dw,
                   int32_t *iw, double *ws, void *stream);
int ipx_qrp_reflectors(int64_t m, int64_t n, int64_t r, const double *W, const double *dw,
                       const int32_t *iw, double *Vp, double *taup, void *stream);
int ipx_qrp_write_t(int64_t m, int64_t n, int64_t r, const double *W, const double *dw,
                    const int32_t *iw, double *T, int64_t ldt, void *stream);
int ipx_qrp_fold_columns(int64_t rows, int64_t m, int64_t ld, const double *in, const int32_t *perm,
                         double *out, void *stream);

/* ---- dense constraint Jacobians with inequality rows (csrc/densejac.hip; device-callback
 * mode's dense canonical form, _canonical_constraint.py:240-280, :363-438, and the barrier's
 * augmented Jacobian, tr_interior_point.py:141-194).  Row-major, explicit leading dimensions.
 * out[dst[r], col0 + j] = sign[r] * src[idx[r], j], r < rows, j < ncols; idx / sign / dst may
 * each be NULL (r, 1, r).  Row selection, re-signing and stacking of several parts. */
int ipx_dense_gather_rows(int64_t rows, int64_t ncols, const double *src, int64_t lds,
                          const int32_t *idx, const double *sign, const int32_t *dst,
                          double *out, int64_t ldo, int64_t col0, void *stream);
/* out[dst[r], 0:ncols] = sign[r] * (row idx[r] of the CSR matrix, densified) */
int ipx_csr_rows_to_dense(int64_t rows, int64_t ncols, const int32_t *rowptr,
                          const int32_t *colidx, const double *val, const int32_t *idx,
                          const double *sign, const int32_t *dst, double *out, int64_t ldo,
                          void *stream);
/* A = [[J_eq, 0], [J_in, diag(s)]], (m_eq + m_in) x (n + m_in), leading dimension n + m_in;
 * At (optional) = A', leading dimension m_eq + m_in, written in the same pass; A may be NULL
 * when At is not (the transpose alone). */
int ipx_dense_augment(int64_t m_eq, int64_t m_in, int64_t n, const double *J_eq, int64_t ld_eq,
                      const double *J_in, int64_t ld_in, const double *s, double *A, double *At,
                      void *stream);
/* G = G0 + diag(0_{m_eq}, s*s) on the M x M layout, M = ipx_dense_padded(m), s[k] at
 * s + k * incs; G0 NULL: in place.  (A A' for A = [[J_eq, 0], [J_in, diag(s)]] from the Gram
 * of its first n columns; s read off A's diagonal block with incs = n + m_in + 1.) */
int ipx_gram_shift(int64_t m, int64_t m_eq, const double *G0, const double *s, int64_t incs,
                   double *G, void *stream);

/* ---- banded SPD solve with S = A A' (normal equations, projections.py:58-90;
 * replaces SuperLU solve :102,120 / CHOLMOD :62).  Partitioned (SPIKE-style)
 * LDL': see csrc/banded.hip.  Half bandwidth <= ipx_banded_kmax(). */
int ipx_banded_kmax(void);
void *ipx_banded_create(int64_t m, int32_t k, int32_t chunk);
void ipx_banded_destroy(void *handle);
int ipx_banded_levels(void *handle);
/* band[d*m+i] = S[i][i-d], d = 0..k; must outlive the solves. */
int ipx_banded_factor(void *handle, const double *band, void *stream);
/* Blocking: IPX_OK; IPX_ENOTSPD when a pivot was <= 0 (rank-deficient A); IPX_EILLCOND when
 * every pivot is positive but one lost 43 bits (solves are available; the Python host takes the
 * reference's SVD exit, projections.py:101-108, when the matrix is small enough for it). */
int ipx_banded_status(void *handle, void *stream);
/* After ipx_banded_status: 1 when the separator system was found diagonal to
 * working precision (|off-diagonal| <= 2^-56 |diagonal|) so solves skip the
 * middle kernel; ipx_banded_set_decoupling(h, 0) forces the full path. */
int ipx_banded_decoupled(void *handle);
int ipx_banded_set_decoupling(void *handle, int allow);
/* k = 1: level (1..7) at which the cyclic reduction of A A' has decoupled -- the single-launch
 * solve is then a parallel cyclic reduction over windows of rows; 0 = chunk recurrences.
 * ipx_banded_set_decoupling(h, 2) switches back to the chunk form (cross-checks);
 * (h, 16 + L) forces the reduction to stop at level L (tests: an inexact solve). */
int ipx_banded_pcr_level(void *handle);
/* After ipx_banded_status: correction steps per solve when the factorization runs defect
 * correction on the single-launch solve (separator blocks coupled and the separator level
 * long or -- half bandwidth 5..8 -- not compiled), else 0; *eta (may be NULL) = measured
 * contraction bound.  ipx_banded_status returns IPX_EUNSUPPORTED for half bandwidth 5..8
 * when the bound is >= 0.5: the caller takes another solver. */
int ipx_banded_refine_steps(void *handle, double *eta);
/* Rows per chunk of level 0 (interior rows + half bandwidth): the last chunk takes the
 * m mod q (or q) rows that are left. */
int ipx_banded_chunk_rows(void *handle);
int ipx_banded_solve(void *handle, const double *w, double *x, void *stream);
/* Same, skipped on the device when *guard != 0 (stop flag of the CG loops). */
int ipx_banded_solve_guarded_c(void *handle, const double *w, double *x, const double *guard,
                               void *stream);
/* One-kernel-per-level variant of the same solve (cross-check / LDS fallback). */
/* After ipx_banded_status: 1 when solves take the single-launch decoupled path; then
 * out[0] = constraint rows per workgroup of that kernel, out[1] = its workgroups. */
int ipx_banded_decoupled_geometry(void *handle, int32_t *out);
/* solve + per-workgroup partials of ||w - (A A') x||^2 (ceil(m/256) doubles). */
int ipx_banded_solve_resid(void *handle, const double *w, double *x, double *partial,
                           int32_t *npartial, const double *guard, void *stream);
int ipx_banded_solve_multilaunch(void *handle, const double *w, double *x, void *stream);
/* band of (P A)(P A)' for CSR A with row order perm (NULL = identity). */
int ipx_aat_band(int64_t m, int32_t k, const int32_t *rowptr, const int32_t *colidx,
                 const double *val, const int32_t *perm, double *band, void *stream);

/* ---- device-resident projected CG (qp_subproblem.py:549-634): see csrc/cg.hip.
 * The argument block holds device pointers only; every member is 8 bytes (but the last one,
 * an int32 flag). */
typedef struct ipx_cg_args {
  int64_t n, m;
  const int32_t *A_rowptr, *A_colidx; const double *A_val; const int32_t *A_tiles; int64_t A_ntiles;
  const int32_t *At_rowptr, *At_colidx; const double *At_val; const int32_t *At_tiles; int64_t At_ntiles;
  const int32_t *H_rowptr, *H_colidx; const double *H_val; const int32_t *H_tiles; int64_t H_ntiles;
  const double *H_diag;
  void *banded;
  double *x, *p, *r, *Hp;
  double *w, *v, *t;
  const double *lb, *ub;
  double *state;
  double *part1, *part2, *part3, *part4;
  int64_t vec_grid;
  int64_t solver_kind;   /* 0: `banded` is an ipx_banded handle; 1: an ipx_boxschur_args*;
                          * 2: dense Jacobian -- A_val / At_val are row-major m x n / n x m matrices
                          * (the index arrays NULL), `banded` is G^-1 (M x M doubles, M = m rounded up
                          * to 32; w and v M long, zero tail), H is CSR or, with H_rowptr NULL, a
                          * row-major n x n matrix in H_val; part1/3/4 hold 2 x 2048 doubles */
  /* step2 fused into the H.p SpMV (banded H): H_hmax > 0 = widest distance of a row tile's
   * columns from its own row range (<= 64, <= rows of every tile), pb = 2 x H_ntiles x
   * 2*H_hmax doubles of scratch (tile-boundary copies of p, by iteration parity).
   * pb == NULL or H_hmax == 0: separate step2 and H.p launches. */
  double *pb;
  int64_t H_hmax;
  int64_t H_tile_rows;   /* rows of H's longest row tile (0 = unknown) */
  /* step1 fused into the A.r SpMV (banded A, no box): A_own = 2*(A_ntiles+1) ints -- the
   * first column each row tile owns (A_ntiles+1 entries, a partition of [0, n)), then one
   * past the last column it touches; A_span = longest own-start-to-last-touched distance
   * (<= 2048); r_next = n doubles of scratch.  Any of them 0 / NULL, or lb given: separate
   * launches. */
  double *r_next;
  const int32_t *A_own;
  int64_t A_span;
  /* IPX_FOLD_WS_DOUBLES doubles of scratch: partial-sum arrays longer than ~1000 entries
   * (n beyond ~1e6) are compacted into it before the consumers fold them; NULL = never. */
  double *fold_ws;
  /* g = r - A'v as the tail of the single-launch decoupled banded solve (tridiagonal A A'):
   * At_vown = workgroups+1 ints, the variables each workgroup of that kernel owns (those
   * whose first constraint lies in its rows; see ipx_banded_decoupled_geometry); At_qv =
   * ceil(most variables of one workgroup / 256) <= 16.  NULL / 0: separate SpMV. */
  const int32_t *At_vown;
  int64_t At_qv;
  int64_t A_tile_nnz;    /* must be 0 (a row-tile table of its own for the fused step1 was an
                          * experiment of round 2; the field keeps the layout) */
  /* the rows of A' once more in ELL(2) form for that tail, indexed by the variable alone (no
   * row-pointer round trip): At_ell_val = 2n doubles, entry t of variable j at [t*n + j], t = 0
   * its FIRST constraint, t = 1 the next row (tridiagonal A A': a variable sees at most two
   * constraints and they are adjacent), an absent entry 0; At_ell_row = n uint16 (n even), the
   * first constraint's row as an offset from the first row of the workgroup that owns the
   * variable (At_vown; < rows per workgroup).  18 bytes per variable.  NULL: CSR. */
  const uint16_t *At_ell_row;
  const double *At_ell_val;
  /* Compact index form of H for the fused step2 + H.p kernel (H_hmax > 0), or NULL:
   * H_col16 = one uint16 per nonzero, its column as an offset into the row tile's span
   * (col - max(tile's first row - H_hmax, 0)); H_rowlen = one int per row tile, the common
   * length of its rows or -1 (then H_rowptr is read for that tile).  Same arithmetic; 2 B
   * instead of 4 per nonzero and no row pointers on uniform tiles.  A uniform, non-empty tile
   * whose entry k of row i has the offset H_col16[tile's first entry] + i + k may carry bit 16
   * (0x10000) in its word: under the radius guard the kernel then forms the tile's offsets and
   * reads that one entry of H_col16 alone; every other form ignores the bit. */
  const void *H_col16;
  const int32_t *H_rowlen;
  /* The same for the fused step1 + A.r kernel (A_span > 0, standard tiles):
   * one uint16 per nonzero of A, col - A_own[its row tile]; NULL: A_colidx is read. */
  const void *A_col16;
  /* != 0: the trust radius in the state block is +inf (and, fused step1 implying no box, the
   * tests of qp_subproblem.py:583,599 can never trigger): ||x + alpha p||^2 is not formed --
   * the fused step1 + A.r kernel then does not read x and p.  Only read when step1 is fused. */
  int64_t no_radius;
  /* Tables of the RESIDENT form of the loop (csrc/resident.hip: a whole batch of iterations in
   * one launch, one workgroup per 260 rows of a tridiagonal A A', all of them co-resident; the
   * per-rank sizes of a multi-GPU run).  For a Jacobian whose rows all have A_rl entries, no
   * box: A_off16 = one uint16 per entry of A (column - first column of its row), A_rowfirst =
   * one int per row, P_win = 2 ints per workgroup of the solve (first column / one past the
   * last column of the span it needs: the columns of its window's rows and its own variables),
   * P_nspan = the longest span (<= 4096), P_navn below; needs At_vown. */
  const void *A_off16;
  const int32_t *A_rowfirst;
  int64_t A_rl;
  const int32_t *P_win;
  int64_t P_nspan;
  int64_t P_navn;        /* most own variables of one workgroup (At_vown differences) */
  /* != 0: the Hessian is an operator the CALLER applies between two iterations (reference
   * _canonical_constraint.py:119-139 allows LinearOperator terms: finite differences, user
   * callbacks): the loop's launches leave out H.p; after every iteration the caller writes
   * Hp = H p and the scalar p'Hp into part1[1] (H_ntiles = 1, the H_* arrays unused).  The
   * branches and step lengths stay on the device. */
  int64_t H_operator;
  /* != 0 with the tables above: ipx_cg_iterate runs a batch as one resident launch when
   * ipx_cg_resident_ok says the sizes fit (every row of H at most 4 entries -- the caller's
   * check --, <= 224 workgroups, spans within the kernel's budgets).  R_ll = the hand-off buffer
   * (ipx_cg_resident_ll_words(workgroups, R_hw) 8-byte words, zeroed once), R_hw = the longest
   * halo (columns of a workgroup's span beyond its own variables, either side), R_seq = a HOST
   * counter owned by the caller (starts at 0; the library advances it by the tags a launch
   * uses).  A launch in which a hand-off timed out records stop code 8 and leaves x, p, r, Hp
   * and the state block untouched: clear the code, set resident = 0 and repeat the batch. */
  int64_t resident;
  void *R_ll;
  int64_t R_hw;
  int64_t *R_seq;
  /* A low-rank term of the Hessian (csrc/lowrank.hip: B = sigma I + W C W' on the first LR_rows
   * rows, zero elsewhere), added by every H.p of the loop behind the CSR / dense / diagonal part
   * -- or alone, H_rowptr and H_val NULL: then H_diag (or nothing) is the rest.  LR_W = the
   * ring buffer (2 LR_mem columns of LR_rows), LR_state = its state block, LR_part =
   * 2 LR_mem x ipx_lowrank_grid(LR_rows) doubles of scratch.  With LR_W set, the p'Hp partials
   * of the final Hp are per workgroup of that product (part1_count: ipx_lowrank_grid(LR_rows),
   * part1 2 x that long); the resident and PEER forms and the outer-iteration chains refuse
   * the block.  LR_W NULL: every launch sequence is unchanged. */
  const double *LR_W;
  const double *LR_state;
  double *LR_part;
  int64_t LR_mem;
  int64_t LR_rows;
  /* Carried sums for the radius test of qp_subproblem.py:583 (both fused kernels in use, no
   * box, finite radius; NULL: the test reads x and p as before).  k_cg_step2_hp of iteration
   * `it` has x_next and p_next on its own rows in registers and leaves per row tile of H the
   * partials of sum x^2, sum x p, sum p^2, and the tag it + 1 ("these sums belong to the x and
   * p iteration it + 1 starts from").  The fused step1 + A.r kernel of iteration it + 1 then
   * reads neither x nor p: its first ceil(H_ntiles / 64) workgroups fold one 64-entry slice of
   * the three arrays each (NaNs when the tag is not `it`), and that
   * iteration's k_cg_step2_hp forms ||x + alpha p||^2 = XX + 2 alpha XP + alpha^2 PP from the
   * folded sums.  It decides :583 only when the sums are this iteration's and the value lies
   * outside a relative band of 1e-9 around radius^2 (IPX_CG_STOP_RADIUS_UNDECIDED otherwise:
   * the host forms the norm).
   * Layout, doubles: [0, 3 H_ntiles) the partials, array by array; [3 H_ntiles] their tag;
   * then three arrays of 256 for the folded sums (ceil(H_ntiles / 64) <= 256 entries used, the
   * rest stays zero) and one spare double: 3 H_ntiles + 770 in all, zeroed once.  More than
   * 16384 row tiles of H (n beyond ~1.1e7 at 3 entries per row): the test reads x and p.
   * Every entry point that changes x or p
   * outside k_cg_step2_hp clears the tag (ipx_cg_hp, ipx_cg_prime, ipx_cg_resume,
   * ipx_cg_save_pb, the resident launch, an ipx_cg_iterate batch with no_radius set).  The
   * stand-alone ipx_cg_step2_hp runs the kernel without the sums and leaves the tag alone: do
   * not set xsums_carry behind it. */
  double *xsums;
  /* The projection half of an iteration as ONE launch (csrc/banded.hip k_step1_solve_tail:
   * step1, w = A r_next, the cyclic-reduction solve and g = r_next - A'v on the solve's windows;
   * two launches per iteration).  fused_proj != 0 asks for it; the library takes it when the
   * fused step1, the solve's tail in its ELL(2) form and the window tables above (A_off16's
   * siblings A_rowfirst, A_rl <= 16, P_win, P_nspan <= 4096) are all bound, n is even, no box,
   * and a resident launch does not apply -- else the three launches, whose tables stay bound.
   * A_ell_val / A_ell_off16 = A once more, ELL-transposed for one lane per row: entry k of row
   * i at [k * m + i], the values and the column as a 16-bit offset from A_rowfirst[i].
   * r_where = one int32 of device memory, zeroed once: within a batch the roles of r and r_next
   * alternate (a workgroup's g must not overwrite entries of r its neighbours' windows still
   * read), the word says where the current r lives and every entry point that enqueues
   * iterations ends with one guarded launch that copies it back.  When an entry point returns,
   * r holds the current residual whatever the iteration count or stop code. */
  int64_t fused_proj;
  const double *A_ell_val;
  const void *A_ell_off16;
  int32_t *r_where;
  /* != 0: the first iteration of the next ipx_cg_iterate call may take the carried sums too
   * -- the caller knows that the previous batch on this block ended exactly there without a
   * stop and that nothing has run on it since.  0: that iteration reads x and p. */
  int32_t xsums_carry;
  /* != 0: entry k of every row of A sits at column A_rowfirst[row] + k (rows are runs of
   * consecutive columns, as on a banded Jacobian): the fused projection takes the offset as the
   * constant k and does not read A_ell_off16 (which stays bound).  0: the table is read. */
  int32_t A_contig;
  /* The radius guard: the test of qp_subproblem.py:583 decided from a norm bound while that bound
   * stays below the radius.  rguard = three doubles of device memory X, Q, T with X >= ||x_k||,
   * Q >= ||p_k|| in floating point (ipx_rguard_step_x / ipx_rguard_step_q below: the triangle
   * inequality on x + alpha p and beta p - g, every update inflated by 1 + 2^-20); T is the
   * bound on ||x_k + alpha p_k|| the projection half of iteration k leaves for its update half.
   * radius_guard != 0 with rguard bound, where the carried sums (xsums) would apply:
   * ipx_cg_iterate runs the kernels of the no_radius loop -- x and p are not read by the
   * projection half, no sums are formed or folded -- plus these scalars on lead lanes; the
   * priming (ipx_cg_prime, ipx_cg_prime_state_guard) writes X0 and Q0.  A bound that is not
   * below the radius (or not finite) stops the batch with IPX_CG_STOP_GUARD_LOST and commits
   * nothing: ipx_cg_guard_resume finishes the iteration in the carried-sum form, and the caller
   * clears radius_guard for the rest of the call.  0 (or rguard NULL): every launch as
   * without the field. */
  double *rguard;
  int32_t radius_guard;
} ipx_cg_args;
/* k_cg_step2_hp mode bits: 1 = no radius / box test, 2 = no orthogonality test (the two
 * ipx_cg_resume and ipx_cg_step2_hp take), 4 = the radius test from the carried sums, 8 = from
 * the radius guard's bound (both set by ipx_cg_iterate alone). */
#define IPX_CG_MODE_NO_RADIUS 1
#define IPX_CG_MODE_NO_ORTH 2
#define IPX_CG_MODE_CARRIED 4
#define IPX_CG_MODE_GUARD 8
/* Stop code 10 of the state block: the carried sums could not decide the radius test (inside
 * the band, or their tag is not this iteration's).  Nothing of the iteration's step2 was
 * committed; the host forms ||x + alpha p|| itself and takes the exit of :583 or resumes
 * (ipx_cg_resume, mode 1). */
#define IPX_CG_STOP_RADIUS_UNDECIDED 10
/* Stop code 11: the radius guard's bound T on ||x + alpha p|| is not below the radius (or not
 * finite).  Nothing of the iteration's step2 was committed; ipx_cg_guard_resume takes over. */
#define IPX_CG_STOP_GUARD_LOST 11
/* The radius guard's arithmetic, shared by the kernels and the host (a CPU test drives the same
 * code): ipx_rguard_step_x = (X + |alpha| Q)(1 + 2^-20) >= ||x + alpha p||,
 * ipx_rguard_step_q = (beta Q + sqrt(gg))(1 + 2^-20) >= ||beta p - g|| with gg = ||g||^2 as the
 * loop summed it, ipx_rguard_start = sqrt(sumsq)(1 + 2^-20) >= the norm a computed sum of squares
 * stands for.  The inflation covers the error of a sum of up to 2^31 squares in any order
 * (<= 2^-22 relative) and the roundings of fl(x + fl(alpha p)), fl(fl(beta p) - g). */
double ipx_rguard_start(double sumsq);
double ipx_rguard_step_x(double X, double Q, double alpha);
double ipx_rguard_step_q(double Q, double beta, double gg);
/* After stop code 11 on iteration it_stop (the stop word cleared by the caller): the sums of
 * x^2, x p, p^2 over the current x and p into the carried sums' folded arrays (256 workgroups,
 * fixed order), then that iteration's update half in the carried-sum form (mode 4, the sums
 * written), then the folded arrays zeroed again (the loop's launches write only their first
 * ceil(H_ntiles / 64) entries).  From there the call runs as with radius_guard = 0, the next
 * batch with xsums_carry = 1 when this launch ends without a stop. */
int ipx_cg_guard_resume(const ipx_cg_args *a, int32_t it_stop, void *stream);
/* ipx_cg_prime_state that also writes X0 and Q0 of the radius guard (rguard: three doubles, or
 * NULL) from ||x0||^2 and rt_g, in the same launch. */
int ipx_cg_prime_state_guard(double *state, const double *red, const int32_t *idx7, double tol_in,
                             double radius, double orth_tol, double norm_A, double cancellation,
                             double *rguard, void *stream);
int ipx_cg_resident_ok(const ipx_cg_args *a);
int64_t ipx_cg_resident_ll_words(int32_t nwg, int32_t hw);
/* the kernel's budgets for the host code that builds its tables: workgroups per launch, threads,
 * span columns / own variables / window rows per workgroup, entries per row of A / of H, halo
 * entries; and the workgroups of all ranks of a sharded launch together */
void ipx_cg_resident_limits(int32_t *out8);
int32_t ipx_cg_resident_max_global(void);
int ipx_cg_state_size(void);
int ipx_cg_vec_grid(int64_t n);
/* Hp = H p (+ diag*p) with p'Hp partials: primes the loop. */
int ipx_cg_hp(const ipx_cg_args *a, void *stream);
/* Enqueue iterations [it_begin, it_end); never synchronises. */
int ipx_cg_iterate(const ipx_cg_args *a, int32_t it_begin, int32_t it_end, void *stream);
/* The state block of a new call from reductions left in device memory (red[idx7[k]], idx < 0:
 * zero): ||x0||^2; ||t||^2, ||r0||^2, ||A r0||^2; ||r0||^2, ||g0||^2, ||A g0||^2 -- rt_g, the
 * tolerance (tol_in, or the rule of qp_subproblem.py:529-530 when tol_in is NaN), radius and
 * orthogonality threshold are written by a one-thread kernel, stop code 9 when a projection
 * needs the host (refinement, cancellation step) or the start is at the trust-region boundary:
 * no host read between a call's priming and its first batch. */
/* The whole priming of a call (qp_subproblem.py:502-512: x0 = Y(-b), r0 = Z(H x0 + c), g0 = Z r0,
 * the state block, p = -g0, Hp = H p) enqueued by ONE call into the loop's own buffers; CSR A
 * (A_tiles / A_ntiles: its standard SpMV row tiles) and H, solver_kind 0 or 1; b NULL = 0;
 * red: 18 doubles, ws: IPX_WS_DOUBLES doubles of device memory.  first_end > 0: iterations
 * [0, first_end) are enqueued behind the priming by the same call (as ipx_cg_iterate would).
 * steps != 0 (b == NULL only): the two projections may each take ONE correction step on the
 * device -- the refinement of projections.py:72-78 / the cancellation step of
 * ipsolver/projector.py, decided from the same norms by a kernel in between (red[14 + j] = 0
 * when projection j takes it, red[16 + j] = 1 once it has; state block: ST_PRIME_STEPS); six more
 * launches, no-ops when none is due.  steps == 0: a projection that needs one ends the priming
 * with stop code 9.  With a tridiagonal A A' on the single-launch solve a projection is the
 * product A x + that solve with z = x - A'v, ||z||^2 and ||A z||^2 (as the residual
 * ||A x - (A A') v||^2: the loop's own measure) from its tail -- two launches.
 * Stop code 9 in the state block afterwards: the host must prime (ipx_cg_prime_state); the
 * iterations enqueued with it did nothing. */
/* doubles of reduction workspace ipx_cg_prime needs for this argument block (the per-tile
 * partials of its six products wait there for one fold); more than IPX_WS_DOUBLES: the entry
 * point returns IPX_EUNSUPPORTED and the caller primes launch by launch. */
int64_t ipx_cg_prime_ws_doubles(const ipx_cg_args *a, int32_t A_ntiles);
int ipx_cg_prime(const ipx_cg_args *a, const int32_t *A_tiles, int32_t A_ntiles, const double *c,
                 const double *b, double *red, double *ws, double tol_in, double radius,
                 double orth_tol, double norm_A, double cancellation, int32_t first_end,
                 int32_t steps, void *stream);
int ipx_cg_prime_state(double *state, const double *red, const int32_t *idx7, double tol_in,
                       double radius, double orth_tol, double norm_A, double cancellation,
                       void *stream);
/* Same launches with HIP events around each kernel class; synchronises once at
 * the end and returns per-class totals in ms_out[0..6] = {step1, A r, banded,
 * r-A'v, A g, step2, H p}.  For per-kernel attribution in bench.py. */
int ipx_cg_iterate_timed(const ipx_cg_args *a, int32_t it_begin, int32_t it_end,
                         float *ms_out, void *stream);
/* The two vector kernels on their own (explicit partial buffers / counts). */
int ipx_cg_step1(int64_t n, double *state, int32_t it, const double *p1, int32_t np1,
                 const double *x, const double *p, double *r, const double *Hp, const double *lb,
                 const double *ub, double *part2, int32_t grid, void *stream);
int ipx_cg_step2(int64_t n, double *state, int32_t it, int32_t mode, const double *p2,
                 int32_t np2, const double *p3, int32_t np3, const double *p4, int32_t np4,
                 double *x, double *p, const double *g, int32_t grid, void *stream);
/* ---- matrix-free (A A')^-1 w: Jacobi-preconditioned CG on A (A' v) = w, device resident
 * (csrc/pcg.hip; replaces the sparse LU of projections.py:93-172 for Jacobians beyond both
 * device factorizations).  State block (doubles): [0],[1] r'z by iteration parity, [2],[3]
 * smallest ||r||, [4],[5] stall counter, [6] done (0 running, 1 converged, 2 fp64 floor,
 * 3 not positive definite), [7] iterations, [8] ||w||, [9] rtol, [10] last ||r||. */
typedef struct ipx_pcg_args {
  int64_t m, n;
  const int32_t *A_rowptr, *A_colidx; const double *A_val; const int32_t *A_tiles; int64_t A_ntiles;
  const int32_t *At_rowptr, *At_colidx; const double *At_val; const int32_t *At_tiles; int64_t At_ntiles;
  const double *dinv;       /* 1 / diag(A A') */
  double *v, *r, *p, *Sp;   /* m-vectors */
  double *t;                /* n-vector: A' p */
  double *state;            /* ipx_pcg_state_size() doubles */
  double *part1, *part2;    /* 2 * A_ntiles and 2 * grid doubles */
  int64_t grid;             /* ipx_cg_vec_grid(m) */
  /* block-Jacobi preconditioner (ipx_blockjacobi_build) or NULL / 0 for the diagonal one:
   * binv = nblk x 32 x 32 inverse blocks, border = 32 nblk row indices (the rows of block b;
   * -1 = padding), z = m doubles (M^-1 r), part3 = nblk / 8 + 1 doubles; dinv is then all zero. */
  const double *binv; const int32_t *border; int64_t nblk;
  double *z, *part3;
  /* coarse level of the two-level preconditioner M^-1 = B^-1 + P X P' (B the blocks above, the
   * columns of P the indicator vectors of groups of consecutive blocks, X = (P' A A' P)^-1), or
   * NULL / 0 for the blocks alone: rsum = nblk doubles (the residual summed per block),
   * coarse_of = m group indices, goff = ncoarse + 1 block offsets of the groups, X = ncoarse x
   * ncoarse at leading dimension ldx (ncoarse <= ipx_pcg_coarse_max()), y = ncoarse doubles
   * (X P'r), partc = ipx_pcg_coarse_grid(ncoarse) doubles. */
  double *rsum; const int32_t *coarse_of, *goff; int64_t ncoarse;
  const double *X; int64_t ldx;
  double *y, *partc;
} ipx_pcg_args;
int ipx_pcg_state_size(void);
int ipx_pcg_iterate(const ipx_pcg_args *a, int32_t it_begin, int32_t it_end, void *stream);
int ipx_pcg_coarse_max(void);
int ipx_pcg_coarse_grid(int64_t ncoarse);
/* z = M^-1 r of the two-level preconditioner described by `a` (binv ... partc; z and r are the
 * arguments, not a->z / a->r) and *rz (device) = r'z, on their own: the first direction of a
 * solve.  Three launches, no-ops when a->state[6] != 0. */
int ipx_pcg_precond_apply(const ipx_pcg_args *a, const double *r, double *z, double *rz,
                          void *stream);
/* Values of C = P'A into the CSR pattern (C_rowptr, C_colidx: per coarse row the sorted union of
 * its member rows' columns): coarse row J = the rows order[32 goff[J]] ... order[32 goff[J+1] - 1]
 * (-1: padding), summed in that order; A's rows have sorted columns. */
int ipx_csr_aggregate_rows(int64_t ncoarse, const int32_t *A_rowptr, const int32_t *A_colidx,
                           const double *A_val, const int32_t *order, const int32_t *goff,
                           const int32_t *C_rowptr, const int32_t *C_colidx, double *C_val,
                           void *stream);
/* Greedy aggregation of the graph of a symmetric pattern S (CSR, n rows, sorted columns), host
 * only: seeds in index order; an aggregate starts as [seed], its member list is walked from the
 * head, every unassigned neighbour of a member (in the column order of its row) is appended and
 * assigned at once while the aggregate has fewer than `cap` members.  agg[i] <- aggregate of row
 * i; returns the number of aggregates, or IPX_EINVAL. */
int ipx_aggregate_greedy(int64_t n, const int32_t *rowptr, const int32_t *colidx, int32_t cap,
                         int32_t *agg);
int ipx_blockjacobi_build(int64_t nblk, const int32_t *rowptr, const int32_t *colidx,
                          const double *val, const int32_t *order, double *binv, int *flag,
                          void *stream);
int ipx_blockjacobi_apply(int64_t m, int64_t nblk, const int32_t *order, const double *binv,
                          const double *r, double *z, double *ws, const double *state,
                          void *stream);
/* ---- partitioned row-sharded loop (ipsolver/sharded.py FusedShardedCG; replaces the
 * per-iteration body of qp_subproblem.py:549-634 on one rank of a node).  `a` describes the
 * rank's extended local problem (own rows / variables + halo copies; solver_kind 0 or 1); the
 * scalars travel through two all-reduced device buffers.  Ranges are in units of the partial
 * arrays' entries (row tiles / solve workgroups) and select the rank's OWN part. */
typedef struct ipx_shard2_ext {
  double *s1;                    /* [2]  s1[1] = p'Hp (own sum, then all-reduced) */
  double *pack;                  /* [4]  ||x+ap||^2, #violations, ||g||^2, ||A g||^2 */
  int64_t nseg;                  /* segments of the local vector space: 1 (x-space) .. 4 (the
                                  * barrier problem's z = [x; s_nl; s_lb; s_ub]), each laid out
                                  * [left halo | own | right halo] */
  int64_t own_lo[4], own_hi[4];  /* own elements per segment, local indices (step1's reductions) */
  int64_t p1_lo[4], p1_hi[4];    /* own row tiles of H per segment                 (part1) */
  int64_t p3_lo[4], p3_hi[4];    /* own entries of part3 (||g||^2 partials) per segment; with
                                  * g = r - A'v fused into the banded solve: its own workgroups,
                                  * segment 0 only */
  int64_t p2_lo, p2_hi;          /* own entries of part2 (row tiles of A with the fused step1;
                                  * every vector chunk otherwise: step1 masks by element) */
  int64_t p4_lo, p4_hi;          /* own workgroups of the (inner) banded solve (part4) */
  /* Peer mailbox (ipx_peer_create) or NULL.  With it the scalars are all-reduced and the halo
   * of g exchanged INSIDE the loop's own launches (the kernels write into the peers' HBM over
   * xGMI); without it the caller all-reduces s1 / pack and exchanges the halo between the
   * phases itself. */
  void *peer;
  int64_t seg_lo[4], seg_hi[4];  /* the segments' local extents [left halo | own | right halo] */
  int64_t send_left[4], send_right[4];   /* own entries the left / right neighbour keeps as halo */
  /* != 0: ipx_cg_shard2_iterate does the two all-reduces and the halo exchange in the PROLOGUES
   * of the kernels that consume them -- 3 launches per iteration instead of 5; the reduced
   * sums are also left in pack.  The GROUP's decision: set it only when ipx_cg_shard2_fusable
   * returned 1 on EVERY rank (the two forms order an iteration's collectives differently);
   * a rank whose own argument block does not allow it gets IPX_EINVAL. */
  int64_t fuse_comm;
  /* RESIDENT form of the sharded loop (csrc/resident.hip, PEER; ipx_cg_shard2_resident): this
   * rank's own blocks [res_wg0, res_wg0 + res_nwg) of its local banded solve are the global
   * workgroups res_gwg0 .. of res_gnwg (all ranks' own blocks in rank order).  Needs the
   * resident tables of the argument block and ipx_peer_attach_resident on e->peer; the GROUP's
   * decision, like fuse_comm. */
  int64_t res_wg0, res_nwg, res_gwg0, res_gnwg;
} ipx_shard2_ext;
/* 1 when this rank's argument block allows fuse_comm (peer set, the fused 16-bit-index kernels
 * and g = r - A'v as the solve's tail for x-space problems, or the box-Schur projection). */
int ipx_cg_shard2_fusable(const ipx_cg_args *a, const ipx_shard2_ext *e);
int ipx_cg_shard2_segment(const ipx_cg_args *a, const ipx_shard2_ext *e, int32_t phase,
                          int32_t it, int32_t mode, void *stream);
/* Iterations [it_begin, it_end), both phases, communication included (needs e->peer): one
 * call per batch, nothing between the iterations on the host. */
int ipx_cg_shard2_iterate(const ipx_cg_args *a, const ipx_shard2_ext *e, int32_t it_begin,
                          int32_t it_end, void *stream);
/* The same batch as ONE resident launch per rank (reference loop: qp_subproblem.py:549-634; the
 * workgroups of all ranks hand their scalars and halos to each other directly, two hops per
 * iteration).  Writes a rank's OWN entries of x, p, r, Hp only: before the host uses the local
 * vectors (an event, the end of the loop, a batch on the separate launches) it synchronises
 * their halos and calls ipx_cg_save_pb.  A wait that times out records stop code 7. */
int ipx_cg_shard2_resident_ok(const ipx_cg_args *a, const ipx_shard2_ext *e);
int ipx_cg_shard2_resident(const ipx_cg_args *a, const ipx_shard2_ext *e, int32_t it_begin,
                           int32_t it_end, void *stream);
/* p at the row-tile boundaries of H for the fused step2 + H.p kernel, from a->p (after p
 * changed behind the loop's back: a halo synchronisation). */
int ipx_cg_save_pb(const ipx_cg_args *a, void *stream);

/* ---- peer mailboxes (csrc/peer.hip): the transport of the sharded loop's two all-reduces
 * (torch.distributed all_reduce in round 2; qp_subproblem.py:556,583,626 are the reduction
 * points) and of its halo exchange, rank to rank through hipIpc-mapped device memory.
 * create -> export (ipx_peer_handle_bytes() bytes) -> hand the blobs around -> import every
 * other rank's -> ipx_peer_ready.  halo_cap: doubles per side a rank may receive. */
int ipx_peer_handle_bytes(void);
void *ipx_peer_create(int32_t rank, int32_t world, int64_t halo_cap);
int ipx_peer_export(void *peer, void *handle_out);
int ipx_peer_import(void *peer, int32_t rank, const void *handle_in);
int ipx_peer_ready(void *peer);
int64_t ipx_peer_halo_capacity(void *peer);
/* Deadline of a kernel's wait for a peer's word (default 10 s); past it the loop records stop
 * code 7 and returns -- never a hung GPU. */
int ipx_peer_set_timeout(void *peer, double seconds);
int ipx_peer_sequence(void *peer, int64_t *out2);
int64_t ipx_peer_fused_launches(void *peer);   /* loop kernels that did a collective in their prologue */
void ipx_peer_destroy(void *peer);
/* `reps` all-reduces (sum) of nq <= 8 doubles back to back: the mailbox path's latency probe. */
int ipx_peer_allreduce(void *peer, int32_t nq, const double *in, double *out, int *failed,
                       int32_t reps, void *stream);
/* The outer loops' collectives through the mailboxes (no torch.distributed call, no upload):
 * all-gather of nq <= 7 scalars per rank, the caller's own in HOST memory (passed to the kernel
 * by value) -> out (device): world * nq doubles in rank order + 2 (an earlier halo exchange
 * timed out on some rank / this all-gather did);
 * halo exchange of nseg <= 4 segments of a local vector (geom: seg_lo, own_lo, own_hi, seg_hi,
 * send_left, send_right per segment, local indices).  Both collective (every rank, same
 * arguments' shapes), neither synchronises; failed: device int, set when a wait timed out. */
int ipx_peer_allgather(void *peer, int32_t nq, const double *vals, double *out, int *failed,
                       void *stream);
int ipx_peer_exchange(void *peer, double *v, int32_t nseg, const int64_t *geom, int *failed,
                      void *stream);
/* `reps` round trips of one tagged word with `partner` (-1: sit the round out; every rank of
 * the group calls it once per round, the sequence numbers advance alike): ticks2[0] = 100 MHz
 * wall-clock ticks of the exchange, ticks2[1] = 1 when a wait timed out (device int64[2]).
 * The cost of one cross-GPU hand-off, measured before a multi-GPU run (bench.py preflight). */
int ipx_peer_pingpong(void *peer, int32_t partner, int32_t reps, long long *ticks2, void *stream);
/* Hand-off buffers of the resident loop kernel between the ranks: attach (allocates `words`
 * 8-byte words -- ipx_cg_resident_ll_words of the largest launch of the group -- uncached,
 * zeroed) -> export_resident -> hand the blobs around -> import_resident every other rank's
 * -> resident_ready (builds the device-side pointer table; 1 when complete). */
int ipx_peer_attach_resident(void *peer, int64_t words);
int ipx_peer_export_resident(void *peer, void *handle_out);
int ipx_peer_import_resident(void *peer, int32_t rank, const void *handle_in);
int ipx_peer_resident_ready(void *peer);
int64_t ipx_peer_resident_launches(void *peer);
int ipx_cg_shard2_fold_hp(const ipx_cg_args *a, const ipx_shard2_ext *e, void *stream);
/* The fused step2 + H.p launch alone (needs pb / H_hmax in the argument block). */
int ipx_cg_step2_hp(const ipx_cg_args *a, int32_t it, int32_t mode, void *stream);
/* Finish iteration `it` after the host handled a stop-5/6 event. */
int ipx_cg_resume(const ipx_cg_args *a, int32_t it, int32_t mode, void *stream);

/* band of (P A) diag(wcol) (P A)' (column weights; wcol NULL = ones). */
int ipx_aat_band_w(int64_t m, int32_t k, const int32_t *rowptr, const int32_t *colidx,
                   const double *val, const int32_t *perm, const double *wcol, double *band,
                   void *stream);

/* ---- analytic elimination of box-like rows of A A' (csrc/boxschur.hip): groups
 * of one or two rows that touch the same shared column (plus a private entry
 * each).  factor: 1x1 / 2x2 inverses, the rows' shared-column entries (alpha)
 * and the Schur column weights 1 - alpha'B^-1 alpha; tsolve: t = B^-1 w on those
 * rows and u[col] = alpha't; vsolve: v = t - B^-1 (alpha * y[col]).  grp (may be NULL):
 * 4 doubles per group, the rows' entries (a_p, s_p, a_q, s_q) for ipx_boxschur_project.
 * grp2 (may be NULL): 2 doubles per group, (s_p, s_q) carrying the signs of (a_p, a_q) -- the
 * same table in half the bytes when every a is +-1 and no s is negative (box rows); bit 1 of
 * *flag is set when that does not hold (bit 0: a block is not positive definite). */
int ipx_pairs_factor(int32_t ng, const int32_t *rowp, const int32_t *rowq, const int32_t *pos_a,
                     const int32_t *pos_s, const double *val, const int32_t *col, double *alpha,
                     double *inv, double *weight_col, int *flag, double *grp, double *grp2,
                     void *stream);
int ipx_pairs_tsolve(int32_t ng, const int32_t *rowp, const int32_t *rowq, const double *inv,
                     const double *alpha, const double *w, double *t, const int32_t *col,
                     double *u, void *stream);
int ipx_pairs_vsolve(int32_t ng, const int32_t *rowp, const int32_t *rowq, const double *inv,
                     const double *alpha, const double *t, const double *y, const int32_t *col,
                     double *v, void *stream);

/* Prepared argument block of one box-Schur (A A')^-1 (all members 8 bytes). */
typedef struct ipx_boxschur_args {
  int64_t m, n, ng, mR;
  const int32_t *rowp, *rowq, *col, *general;
  const double *inv, *alpha;
  const int32_t *AR_rowptr, *AR_colidx; const double *AR_val; const int32_t *AR_tiles; int64_t AR_ntiles;
  const int32_t *ARt_rowptr, *ARt_colidx; const double *ARt_val; const int32_t *ARt_tiles; int64_t ARt_ntiles;
  void *inner;                       /* ipx_banded handle of the Schur complement */
  double *t, *u, *wR, *rhs, *vR, *y; /* scratch: m, n, mR, mR, mR, n doubles */
  /* group tables for ipx_boxschur_project (NULL: only ipx_boxschur_solve is available):
   * gcol = 3 ints per group (shared column, private column of row p, of row q; -1: the row
   * has none, -2 in the q slot: single-row group),
   * grp = 4 doubles per group (a_p, s_p, a_q, s_q; written by ipx_pairs_factor),
   * gen_cols = the ngen columns that belong to no group, ny = 1 + last column A_R touches,
   * up = n doubles of scratch (zero beyond ny). */
  const int32_t *gcol; const double *grp; const int32_t *gen_cols; int64_t ngen;
  int64_t ny;
  double *up;
  /* optional compact tables for the CG loop's two group kernels (NULL: the forms above):
   * grp2 = ipx_pairs_factor's compact group table (only when its flag bit 1 stayed clear);
   * yell_col / yell_val = the columns of A_R once more, per ITEM of the projection (the ng
   * groups by their shared column, then the ngen other columns) in ELL(2) form: entry t of
   * item i at [t * (ng + ngen) + i], an absent entry = a valid row with value 0.  Indexed by
   * the item alone, the loads need no column -> row pointer -> entries round trip.  Only when
   * no such column holds more than two entries. */
  const double *grp2;
  const int32_t *yell_col; const double *yell_val;
  /* gaffine != 0 (with grp2): group g has the columns (gc0 + g, gc0 + g + gdp, gc0 + g + gdq)
   * and gen_cols[k] = gen0 + k -- every variable bounded on both sides, the usual
   * BoxConstraint; the two kernels compute the columns instead of reading gcol / gen_cols. */
  int64_t gaffine, gc0, gdp, gdq, gen0;
  /* AR_rowlen = 2, 4, 8 or 16 when EVERY row of A_R has that many entries (entry j of row i at
   * AR_colidx / AR_val [i * AR_rowlen + j]), else 0: ipx_boxschur_project then forms A_R u
   * inside the Schur solve's kernel (cyclic-reduction path) instead of by an SpMV launch. */
  int64_t AR_rowlen;
  /* optional (with AR_rowlen, grp2, gaffine, yell_*): ipx_boxschur_project does the per-item
   * back substitution as the TAIL of the Schur solve's kernel instead of in a launch of its own
   * (4 -> 3 launches per CG iteration of the barrier problem).  post_own_g / post_own_e =
   * (workgroups of the solve + 1) ints each: the range of groups / of other columns whose
   * FIRST general row lies in a workgroup's post_rows_wg rows; post_reach = the largest
   * distance from an item's first general row to its second.  NULL: the separate launch. */
  const int32_t *post_own_g, *post_own_e;
  int64_t post_rows_wg, post_reach;
} ipx_boxschur_args;
/* v = (A A')^-1 w; partial (optional, ceil(mR/256) doubles) receives the residual partials. */
int ipx_boxschur_solve(const ipx_boxschur_args *a, const double *w, double *v, double *partial,
                       int32_t *npartial, const double *guard, void *stream);
/* g = r - A'(A A')^-1 A r (the CG loop's projection; g may alias r) with the simple rows
 * handled per group on r itself instead of as matrix rows: 6 launches and ~1/3 of the traffic
 * of  A r -> ipx_boxschur_solve -> r - A'v.  part_g: 2 x ipx_boxschur_project_count(a) doubles
 * (||g||^2 partials; second half zero), part_res / npart_res as ipx_boxschur_solve's. */
int ipx_boxschur_project_count(const ipx_boxschur_args *a);
int ipx_boxschur_project(const ipx_boxschur_args *a, const double *r, double *g, double *part_g,
                         int32_t *npart_g, double *part_res, int32_t *npart_res,
                         const double *guard, void *stream);

/* Deferred form of ipx_banded_status (no blocking read): the verdict of the previous, clean
 * factorization on this handle is ASSUMED for the one just enqueued; a one-thread kernel writes
 * verdict[0] = 0 when the flags agree, else 1 (then: ipx_banded_status, and repeat the solves).
 * IPX_EUNSUPPORTED: nothing to assume on this handle. */
int ipx_banded_status_deferred(void *handle, double *verdict, void *stream);
/* A numeric refresh in THREE launches on a handle that qualifies for the deferred verdict
 * (tridiagonal A A', rows in their own order): the band of A A' (wcol: column weights or NULL),
 * the cyclic reduction's check of the matrix alone, the verdict kernel.  The chunked LDL' that the
 * cyclic-reduction solves never read is left out; a solve that needs it runs it first, with
 * ipx_banded_status' blocking verdict.  Returns 1: done, read `verdict` as above; 0: the handle
 * does not qualify and NOTHING was enqueued (ipx_aat_band_w + ipx_banded_factor +
 * ipx_banded_status); < 0: error. */
int ipx_banded_refactor(void *handle, int64_t m, int32_t k, const int32_t *rowptr,
                        const int32_t *colidx, const double *val, const double *wcol,
                        double *band, double *verdict, void *stream);

/* ---- one outer iteration of the trust-region SQP method as three chains of launches whose
 * decisions are taken on the device (csrc/sqp.hip; reference equality_constrained_sqp.py:102-250,
 * the Newton point of modified_dogleg qp_subproblem.py:366-373, projected_cg :416-643).
 * Every chain ends in a reduction whose last workgroup to arrive folds the partial sums in their
 * fixed order, decides, and writes the scalar block q (ipx_sqp_block_size() doubles, layout in
 * csrc/sqp.hip SQ_*, mirrored by ipsolver/sqp_chain.py); the host reads the block once per chain
 * (host_block: the kernel hands it over itself).  CSR Jacobian and Hessian, banded or box-Schur solver (solver_kind 0 / 1
 * of the CG loop's argument block), constraint rows in the projector's own order. */
typedef struct ipx_sqp_args {
  int64_t n, m;
  const ipx_cg_args *cg;            /* the CG loop's block: A, A', H, the solver, its buffers;
                                     * cg->lb / cg->ub must be lbt / ubt below (or NULL) */
  const int32_t *A_tiles;           /* standard SpMV row tiles of A */
  int64_t A_ntiles;
  double *q;                        /* the block */
  const double *x, *c, *b;          /* iterate (n), gradient (n), constraint value (m) */
  const double *lb, *ub;            /* trust_lb / trust_ub of the step (n) or NULL */
  const double *scale;              /* diagonal of S (n) or NULL */
  double *dn, *ct, *lbt, *ubt, *d, *Hd, *x_next;   /* n each (lbt / ubt NULL with lb / ub) */
  double *Ad;                       /* m */
  double *v_out;                    /* m: the multipliers ipx_sqp_refresh writes */
  double *part;                     /* ipx_sqp_part_doubles() doubles of partial sums */
  double *red, *ws;                 /* 16 doubles / IPX_WS_DOUBLES of scratch (ipx_cg_prime) */
  double orth_tol, cancellation;    /* of the projections (ipx_cg_prime) */
  const double *verdict;            /* device: ipx_banded_status_deferred's word, or NULL */
  const double *A_norm_part;        /* ipx_norms_partials over A's values (ipx_sqp_refresh folds
                                     * them into the block's ||A||_F^2), or NULL */
  int64_t A_norm_grid;
  double *host_block;               /* HOST memory, ipx_sqp_block_size() doubles, or NULL.  Non-NULL:
                                     * ipx_sqp_front / _model / _judge / _refresh return when the
                                     * block has arrived there -- the workgroup that completes the
                                     * block publishes it (no read-back launch behind the chain).
                                     * NULL: the entry returns behind its last launch; the block
                                     * stays in q -- a later chain's block carries all of it (the
                                     * caller enqueues the user's callbacks and ipx_sqp_judge
                                     * behind ipx_sqp_front and reads once) */
} ipx_sqp_args;
int ipx_sqp_block_size(void);
int64_t ipx_sqp_part_doubles(const ipx_sqp_args *s);
/* normal step (have_dn == 0: the Newton point, accepted on the device -- block entry
 * NORMAL_KIND 1 -- or not; then, with_dogleg != 0, the dogleg proper of qp_subproblem.py:375-413
 * behind it on the device -- NORMAL_KIND 2 --, else 0: the caller computes the dogleg step into
 * s->dn and calls again with have_dn = 1), c_t = H dn + c, shifted bounds, the projected CG's
 * priming with the tangential radius of the block and iterations [0, first_end), then
 * ipx_sqp_model.  (with_dogleg costs nine launches that do nothing when the Newton point stands:
 * the caller sets it when the last normal step was not the Newton point.)  with_steps != 0: the
 * priming's two projections may each take one correction step on the device (eight more
 * launches, no-ops when none is due; without them such a priming ends in stop code 9). */
int ipx_sqp_front(const ipx_sqp_args *s, int have_dn, int with_dogleg, int with_steps,
                  double radius, double penalty, double f, double norm_b, double tr_factor,
                  double box_factor, double tol_in, double norm_A, int32_t first_end,
                  void *stream);
/* the CG loop's trust-region / negative-curvature exits (:565-576, :585-596), d = dn + dt,
 * x_next = x + S d, the five sums and the model / penalty / predicted reduction (:135-153);
 * host_cg != 0: the caller finished the CG loop itself (exits included), dt = cg->x as it is */
int ipx_sqp_model(const ipx_sqp_args *s, double penalty, double f, double norm_b, int host_cg,
                  void *stream);
/* ||b_next||, actual / predicted, second-order-correction test, trust-radius ladder, accept
 * (:156-242); f_next by value or, f_next_dev non-NULL, a device scalar */
int ipx_sqp_judge(const ipx_sqp_args *s, const double *b_next, double f_next,
                  const double *f_next_dev, void *stream);
/* v = -(A A')^-1 A c, ||c + A'v||_inf, ||b||_inf, ||b|| (:83-87, 226-239), ||A||_F^2 */
int ipx_sqp_refresh(const ipx_sqp_args *s, void *stream);
/* measurement aid: on != 0 starts bracketing the projected CG's priming + first batch inside
 * ipx_sqp_front with HIP events; on == 0 stops, synchronises and returns their GPU time (ms) and
 * count since the start (the in-solve projected-CG rate of the benchmark) */
int ipx_sqp_cg_timing(int on, double *ms_total, int *calls);
/* the decisions' scalar arithmetic on a HOST copy of the block (the same code the kernels run) */
void ipx_sqp_model_host(double *q);
void ipx_sqp_ratio_host(double *q);
void ipx_sqp_radius_host(double *q);
/* box_sphere_intersections' scalar tail (qp_subproblem.py:99-149,194-234,286-296) from the seven
 * sums of ipx_box_sphere_reduce: out3 = (ta, tb, intersect) */
void ipx_sqp_box_sphere_host(const double *sums7, double radius, int entire_line, double *out3);

/* ---- limited-memory quasi-Newton Hessians (csrc/lowrank.hip, ipsolver/quasi_newton.py) ----
 * B = sigma I + W C W' with W = [S Y]: two rings of `mem` columns (column j at W + j n; slot t
 * holds s_t in column t and y_t in column mem + t; unwritten columns zero), C (2 mem)^2 doubles.
 * State block (ipx_lowrank_state_doubles, zero but for [0] = the initial sigma):
 *   [0] sigma, [1] stored pairs, [2] next slot, [3] updates, [4] skipped, [5] sigma fixed,
 *   [6] the last update stored its pair, [7] that slot, [IPX_LR_HDR...] the Gram W'W, then C
 *   (both 2 mem x 2 mem, row major).
 * kind 0: L-BFGS (Byrd, Nocedal & Schnabel 1994 compact form; stored when s'y > threshold
 * ||s|| ||y||), kind 1: L-SR1 (stored when |s'(y - Bs)| >= threshold ||s|| ||y - Bs|| and the
 * middle matrix inverts with every pivot above 1e-14 max|entry|).  init_scale <= 0: sigma from
 * the pairs ('auto'). */
#define IPX_LR_MAX_MEMORY 32
#define IPX_LR_HDR 16
int64_t ipx_lowrank_state_doubles(int32_t mem);
/* workgroups of the update's and the product's partial sums, and the scratch they need */
int ipx_lowrank_grid(int64_t n);
int64_t ipx_lowrank_part_doubles(int64_t n, int32_t mem);
/* one update with the pair (s, y): s'W, y'W, s's, s'y, y'y in one multi-dot kernel, the skip
 * rule + middle matrix + C in one single-workgroup kernel, s and y copied into their slot when
 * stored; s's == 0 changes nothing (not counted).  Three launches, no read-back. */
int ipx_lowrank_update(int32_t kind, int64_t n, int32_t mem, double init_scale, double threshold,
                       double *W, const double *s, const double *y, double *state, double *part,
                       void *stream);
/* out = sigma p + W C W'p (accumulate != 0: added to out); two launches, out != p */
int ipx_lowrank_apply(int64_t n, int32_t mem, const double *W, const double *state, const double *p,
                      double *out, int32_t accumulate, double *part, void *stream);
/* the update's middle-matrix step on a HOST state block from the folded sums
 * dots = (s'W [2 mem], y'W [2 mem], s's, s'y, y'y): the same arithmetic as the kernel */
void ipx_lowrank_middle_host(int32_t kind, int32_t mem, double init_scale, double threshold,
                             double *state, const double *dots);
/* The y of a pair when the memory also approximates constraint Hessians (one memory for the
 * Lagrangian terms declared with a strategy, ipsolver/quasi_newton.py LagrangianQN): for every
 * variable j
 *   y[j] = ((accumulate ? y[j] : 0) + (base_new ? base_new[j] - base_old[j] : 0))
 *          + sum_k v[t_rowidx[k]] * (val_new[t_perm[k]] - val_old[t_perm[k]])
 * k over row j of the TRANSPOSED pattern of an m x n Jacobian (n rows, nnz entries; t_perm: the
 * position of entry k in the Jacobian's own value array; t_tiles: ipx_csr_tiles_host of
 * t_rowptr) in stored order, the sum started from 0, plain operations.  val_new / val_old: the
 * Jacobian's values at the new and the previous point, on one pattern; base_new / base_old: both
 * or neither (the objective's gradients).  One launch, no atomics; rows longer than a tile keep
 * the same order.  The _host twin runs the same per-row routine on host arrays (and checks the
 * index arrays: IPX_EINVAL). */
int ipx_csr_tdiff_dot(int64_t n, int64_t m, int64_t nnz, const int32_t *t_rowptr,
                      const int32_t *t_rowidx, const int64_t *t_perm, const int32_t *t_tiles,
                      int32_t t_ntiles, const double *val_new, const double *val_old,
                      const double *v, const double *base_new, const double *base_old, double *y,
                      int32_t accumulate, void *stream);
int ipx_csr_tdiff_dot_host(int64_t n, int64_t m, int64_t nnz, const int32_t *t_rowptr,
                           const int32_t *t_rowidx, const int64_t *t_perm, const double *val_new,
                           const double *val_old, const double *v, const double *base_new,
                           const double *base_old, double *y, int32_t accumulate);

/* ---- sparse finite-difference Jacobians (csrc/fdjac.hip, ipsolver/fd_jacobian.py) ----
 * Curtis-Powell-Reid grouped differences of a constraint function on a fixed CSR pattern
 * (reference _numdiff.py:15-103, 484-561).  method: 0 '2-point', 1 '3-point', 2 'cs'; one_sided
 * are bytes (0 / 1); groups[n] holds the group of every column.  Every value is computed with the
 * reference's operations in the reference's order (elementwise, one rounding each): the results
 * are its bits.  The *_host entries run the same inline functions on host arrays.
 *
 * steps: h = (rel * sign(x0)) * max(1, |x0|) with sign(0) = +1 (rel_vec, when not NULL, gives rel
 * per variable), then _adjust_scheme_to_bounds with num_steps = 1: '1-sided' for method 0,
 * '2-sided' for method 1, nothing for method 2.  lb / ub NULL: no bound on that side. */
int ipx_fd_steps(int64_t n, int32_t method, double rel, const double *rel_vec, const double *x0,
                 const double *lb, const double *ub, double *h, unsigned char *one_sided,
                 void *stream);
void ipx_fd_steps_host(int64_t n, int32_t method, double rel, const double *rel_vec,
                       const double *x0, const double *lb, const double *ub, double *h,
                       unsigned char *one_sided);
/* the perturbed point(s) of group g, whole vectors: method 0: x1 = x0 + h [groups == g];
 * method 1: x1 / x2 by the one-sided and central rules; method 2: x1 = h [groups == g] (the
 * imaginary part of the complex point; x2 unused).  dx[j] is written for the members of g only
 * (x1 - x0, x2 - x0 or x2 - x1, from the perturbed point; h for method 2). */
int ipx_fd_perturb(int64_t n, int32_t method, int32_t g, const int32_t *groups, const double *x0,
                   const double *h, const unsigned char *one_sided, double *x1, double *x2,
                   double *dx, void *stream);
void ipx_fd_perturb_host(int64_t n, int32_t method, int32_t g, const int32_t *groups,
                         const double *x0, const double *h, const unsigned char *one_sided,
                         double *x1, double *x2, double *dx);
/* val[k] = df / dx[col[k]] for every stored entry k whose column's group lies in [g_lo, g_hi),
 * one launch over the pattern's SpMV row tiles (ipx_csr_tiles_host); other entries are left as
 * they are.  F1 / F2: (g_hi - g_lo) planes of m function values, plane g - g_lo = the values at
 * group g's perturbed point(s) (F2 for method 1 only; F1 the imaginary parts for method 2). */
int ipx_fd_assemble(int64_t m, int64_t n, const int32_t *rowptr, const int32_t *colidx,
                    const int32_t *tiles, int32_t ntiles, int32_t method, const int32_t *groups,
                    int32_t g_lo, int32_t g_hi, const double *f0, const double *F1,
                    const double *F2, const double *dx, const unsigned char *one_sided,
                    double *val, void *stream);
void ipx_fd_assemble_host(int64_t m, int64_t n, const int32_t *rowptr, const int32_t *colidx,
                          int32_t method, const int32_t *groups, int32_t g_lo, int32_t g_hi,
                          const double *f0, const double *F1, const double *F2, const double *dx,
                          const unsigned char *one_sided, double *val);
/* the symmetric assemble of a finite-difference Hessian (m = n; the pattern structurally
 * symmetric; f0 / F1 / F2 values of the differenced gradient): with q_ij the quotient
 * ipx_fd_assemble writes at (i, j), every stored entry k = (i, j) gets
 *     val[slot ? slot[k] : k] (+)= 0.5 * q_ij [group(j) in range] + 0.5 * q_ji [group(i) in range]
 * An entry both of whose groups are >= g_lo is written (added to when `accumulate`), any other
 * is added to: chunks [g_lo, g_hi) launched in ascending order give the single launch's bits, and
 * `slot` + `accumulate` add several terms into one value array on the union of their patterns
 * (each launch touches a slot once).  Entries with neither group in range are left alone. */
int ipx_fd_assemble_sym(int64_t n, const int32_t *rowptr, const int32_t *colidx,
                        const int32_t *tiles, int32_t ntiles, int32_t method,
                        const int32_t *groups, int32_t g_lo, int32_t g_hi, const double *f0,
                        const double *F1, const double *F2, const double *dx,
                        const unsigned char *one_sided, const int32_t *slot, int32_t accumulate,
                        double *val, void *stream);
void ipx_fd_assemble_sym_host(int64_t n, const int32_t *rowptr, const int32_t *colidx,
                              int32_t method, const int32_t *groups, int32_t g_lo, int32_t g_hi,
                              const double *f0, const double *F1, const double *F2,
                              const double *dx, const unsigned char *one_sided,
                              const int32_t *slot, int32_t accumulate, double *val);

/* ---- block-tridiagonal direct solve with S = A A' (csrc/blocktri.hip): block cyclic reduction
 * for half bandwidths past ipx_banded_kmax() up to ipx_blocktri_kmax() = 64.  S (rows in the
 * order `perm`, NULL = identity) is taken as block tridiagonal in blocks of b = 16, 32 or 64
 * (b >= half bandwidth k), N = ceil(m / b) block rows, the padded tail rows with a unit
 * diagonal.  The caller owns all storage: `ws` holds ipx_blocktri_ws_doubles(m, b) doubles,
 * [D | E | V | diag0 | r | y]: N b^2 doubles each for D, E, V (row-major b x b blocks; after the
 * factorization the Cholesky factor's blocks), N b each for the rest (the solve's work vectors
 * among them: solves on one `ws` are ordered by the stream).  Nothing is allocated and no handle
 * is kept.  Fixed-order fp64: the same values give the same bits. */
int ipx_blocktri_kmax(void);
int64_t ipx_blocktri_ws_doubles(int64_t m, int32_t b);
/* out[0] = levels of the reduction (1 + ceil(log2 N): the last block counts as one), out[1] =
 * the number of surviving block rows at which one workgroup takes all remaining levels in a
 * single launch; returns how many levels run as launches of their own before that (>= 0), or
 * IPX_EINVAL.  Launches: factor 2 + 2 x that, solve 2 + 2 x that. */
int ipx_blocktri_levels(int64_t m, int32_t b, int32_t out[2]);
/* D[I] = S[I, I], E[I] = S[I, I - 1] (E[0] = 0), N blocks each and nothing past them; entries
 * further than k from the diagonal are written as zeros without being formed.  CSR rows sorted,
 * every (row, column) once, as for ipx_aat_band_w: repeated entries are summed by the caller
 * before this (DeviceCSR.from_scipy does), the join does not sum them.  A merge join per entry,
 * products added in column order. */
int ipx_aat_blocktri(int64_t m, int32_t b, int32_t k, const int32_t *rowptr,
                     const int32_t *colidx, const double *val, const int32_t *perm, double *D,
                     double *E, void *stream);
/* Factor the blocks D, E (left as they are -- unless D == ws and E == ws + N b^2: in place, no
 * copy).  flag[0] (cleared first): bit 0 -- a pivot fell below 2^-43 of its original diagonal
 * entry (numerically rank deficient; the factorization is complete); bit 2 (with bit 0) -- a
 * pivot was <= 0 (not positive definite; the factors are not usable). */
int ipx_blocktri_factor(int64_t m, int32_t b, const double *D, const double *E, double *ws,
                        int *flag, void *stream);
/* x = S^-1 w (m entries, in the order of `perm`; w and x may not alias; nothing past x[m - 1]
 * is written): triangular solves with the factor's blocks, backward stable. */
int ipx_blocktri_solve(int64_t m, int32_t b, double *ws, const double *w, double *x,
                       void *stream);

/* ---- the same for half bandwidths past ipx_blocktri_kmax() up to ipx_blockwide_kmax() = 256
 * (csrc/blocktri.hip, second part): blocks of b = 128 or 256 (anything else: IPX_EINVAL), worked
 * on as tiles of 64 x 64 in global memory.  Storage, pivot signals and every contract as for the
 * ipx_blocktri_* calls above, `ws` holding ipx_blockwide_ws_doubles(m, b) doubles. */
int ipx_blockwide_kmax(void);
int64_t ipx_blockwide_ws_doubles(int64_t m, int32_t b);
/* out[0] = levels of the reduction, out[1] = 1 (there is no one-workgroup tail: every level is
 * launched on its own); returns out[0] - 1, or IPX_EINVAL.  Launches: factor 2 + 3 x that,
 * solve 2 + 2 x that. */
int ipx_blockwide_levels(int64_t m, int32_t b, int32_t out[2]);
int ipx_aat_blockwide(int64_t m, int32_t b, int32_t k, const int32_t *rowptr,
                      const int32_t *colidx, const double *val, const int32_t *perm, double *D,
                      double *E, void *stream);
int ipx_blockwide_factor(int64_t m, int32_t b, const double *D, const double *E, double *ws,
                         int *flag, void *stream);
int ipx_blockwide_solve(int64_t m, int32_t b, double *ws, const double *w, double *x,
                        void *stream);

/* ---- bordered direct solve with S = A A' (csrc/bordered.hip): A = [B | C], C the p dense columns
 * (1 <= p <= ipx_border_pmax() = 32), S = S_B + C C' by the Woodbury identity on top of a direct
 * solve with S_B = B B':  S^-1 w = u - Y z,  u = S_B^-1 w,  Y = S_B^-1 C,  K = I + C' Y,
 * K z = Y' w.  C and Y are column-major m x p, K and its Cholesky factor L row-major p x p.  The
 * caller owns all storage and runs the inner solves; nothing is allocated, no handle is kept.
 * Rows are dealt to workgroups in chunks of ipx_border_rows_per_group(); the partial sums of a
 * launch are ipx_border_groups(m) blocks, always added in ascending order (no atomics): the same
 * values give the same bits. */
int ipx_border_pmax(void);
int ipx_border_rows_per_group(void);
/* number of partial blocks of ipx_border_gram (p * p doubles each) and ipx_border_tdot (p each):
 * min(ceil(m / rows_per_group), 512); IPX_EINVAL for m < 1 */
int ipx_border_groups(int64_t m);
/* C = 0, then C[dst[i]] = val[src[i]] for i < nnz (dst = row + m * border column; every
 * (row, column) once, dst[i] < m * p: the caller's index lists, made once per pattern) */
int ipx_border_scatter(int64_t m, int32_t p, int64_t nnz, const double *val, const int32_t *src,
                       const int64_t *dst, double *C, void *stream);
/* part[g] = the p x p block of C' Y over the rows of group g */
int ipx_border_gram(int64_t m, int32_t p, const double *C, const double *Y, double *part,
                    void *stream);
/* K = I + sum_g part[g] (all p * p entries written; the lower triangle is what is factored),
 * L = its Cholesky factor (zeros above the diagonal), by one workgroup in LDS.  info[0]: bit 0 --
 * a pivot fell below 2^-43 of its diagonal entry; bit 2 (with bit 0) -- a pivot was <= 0;
 * info[1] = trace(K).  `m` selects the number of partial blocks only. */
int ipx_border_chol(int64_t m, int32_t p, const double *part, double *K, double *L, double *info,
                    void *stream);
/* part[g] = the p partial sums of t = Y' w over the rows of group g */
int ipx_border_tdot(int64_t m, int32_t p, const double *Y, const double *w, double *part,
                    void *stream);
/* z = (L L')^-1 (sum_g part[g]), v[r] = u[r] - sum_j Y[r, j] z[j]; v may be u */
int ipx_border_apply(int64_t m, int32_t p, const double *Y, const double *L, const double *part,
                     const double *u, double *v, void *stream);

/* ---- linked direct solve with S = A A' (csrc/linked.hip): the rows of A are m_B band rows B and
 * q link rows D (1 <= q <= ipx_border_pmax(), m = m_B + q, m_B >= 1), in any positions:
 *     S = [S_B E; E' F],  S_B = B B',  E = B D',  F = D D',  Y = S_B^-1 E,  K = F - E' Y,
 *     u = S_B^-1 w_B,  K z = w_D - Y' w_B,  v_B = u - Y z,  v_D = z.
 * The caller owns all storage and runs the inner solves; nothing is allocated, no handle is kept.
 * Layouts: Dt = D' is n x q ROW-major (entry (c, j) at c * q + j; ipx_border_scatter(n, q, ...)
 * with dst = column * q + link row fills it), so that the q lanes of a row read q adjacent
 * doubles per entry of A.  G and Y are column-major m x q with leading dimension m; rows
 * 0 .. m_B - 1 of G are E, rows m_B .. m - 1 are F; the same rows of Y are S_B^-1 E and ZEROS,
 * and the gathered w_B carries q zeros at its end: ipx_border_gram(m, q, G, Y, part) and
 * ipx_border_tdot(m, q, Y, w_B, part) then give the partial blocks of E' Y and Y' w_B in place
 * (ipx_border_groups(m) of them).  K and L are row-major q x q.  Fixed-order fp64, no atomics: the
 * same values give the same bits. */
/* G[dst_row[r] + m j] = sum over the entries e of row r of A (m x n CSR), in storage order, of
 * val[e] * Dt[colidx[e] * q + j]: one multiply and one add per entry, A read once for all q.
 * dst_row: band rows to 0 .. m_B - 1, link rows to m_B .. m - 1 (a permutation of 0 .. m - 1;
 * the product itself takes any permutation and any m >= 1). */
int ipx_link_spmm(int64_t m, int64_t n, int32_t q, const int32_t *rowptr, const int32_t *colidx,
                  const double *val, const double *Dt, const int32_t *dst_row, double *G,
                  void *stream);
/* K = F - sum_g part[g] (ascending g; all q * q entries written, the lower triangle is what is
 * factored), L = its Cholesky factor (zeros above the diagonal), by one workgroup in LDS.
 * info[0]: bit 0 -- a pivot fell below 2^-43 of F_jj, the diagonal entry of S; bit 2 (with
 * bit 0) -- a pivot was <= 0; info[1] = max_j F_jj / K_jj (infinite for a K_jj <= 0). */
int ipx_link_chol(int64_t m, int32_t q, const double *G, const double *part, double *K, double *L,
                  double *info, void *stream);
/* t = w[d_rows] - sum_g part[g] (the order of ipx_border_apply), z = (L L')^-1 t,
 * v[b_rows[r]] = u[r] - sum_j Y[r, j] z[j] (r < m_B, j ascending), v[d_rows[j]] = z[j]: v in the
 * caller's row order, w the caller's right-hand side; v may alias neither w nor u. */
int ipx_link_apply(int64_t m, int32_t q, const double *Y, const double *L, const double *part,
                   const double *u, const double *w, const int32_t *b_rows, const int32_t *d_rows,
                   double *v, void *stream);

/* ---- sparse direct solve with S = A A' for any pattern (csrc/nested_order.hip, csrc/nested.hip):
 * nested dissection, a supernodal multifrontal Cholesky factorization, level by level.
 *
 * Host graph work (no device call).  The pattern of S is symmetric CSR with sorted columns.
 * ipx_nd_order: a part (ascending rows) of at most `leaf` rows is one supernode.  A larger part
 * that is not connected goes piece by piece, the pieces in the order of their lowest rows.  A
 * connected part larger than `leaf`: breadth-first levels from its lowest row, restarted twice
 * from the lowest row of the last level; fewer than three levels: one supernode; else the
 * separator is the first level at which the cumulative count reaches half the part (rounded up),
 * clamped to 1 ... levels - 2; the rows before it are ordered first, then the rows after it, then
 * the separator as one supernode.  Rows inside a supernode ascend.  perm (n): position -> row;
 * sn_ptr (n + 1 slots, count + 1 used): the supernodes' ranges of positions.  Returns the number
 * of supernodes. */
int ipx_nd_order(int64_t n, const int32_t *rowptr, const int32_t *colidx, int32_t leaf,
                 int32_t *perm, int32_t *sn_ptr);
/* ipx_nd_symbolic: per supernode its boundary -- the later positions it couples to after fill,
 * ascending, bnd[bnd_ptr[j] .. bnd_ptr[j + 1]) --, its parent in the elimination tree (the owner
 * of the first boundary position; -1: a root), its level (0 without children, else one more than
 * the highest child's; children are the supernodes j' < j with parent j, ascending) and, beside
 * every boundary position, its index in the parent's front (the parent's own positions, then its
 * boundary): cmap.  Returns the total boundary length; bnd and cmap are filled only when they
 * are given and `cap` holds it (call once with bnd = NULL for the size). */
int64_t ipx_nd_symbolic(int64_t n, const int32_t *rowptr, const int32_t *colidx, int32_t nsuper,
                        const int32_t *perm, const int32_t *sn_ptr, int32_t *parent,
                        int32_t *level, int64_t *bnd_ptr, int32_t *bnd, int32_t *cmap,
                        int64_t cap);

/* Device side.  A front is the square matrix over a supernode's s own rows and its b boundary
 * rows, stored ROW-major with leading dimension ld, lower triangle: after the factorization
 * rows 0 .. s - 1 hold L11, the boundary rows (from row s + pad on) hold L21 in columns
 * 0 .. s - 1 and the update matrix F22 - L21 L21' behind them; above the diagonal, rows
 * 0 .. s - 1 hold the same columns of L once more (L' -- what the forward solve reads).  A front of at most
 * ipx_nd_small_max() rows may be "small": ld = s + b, pad = 0, factored by one workgroup out of
 * LDS.  Any front may be "large": the own rows padded to a multiple of 64 by unit diagonal
 * (pad), ld the next multiple of 64 of s + pad + b, factored by 64 x 64 tiles
 * (ipx_chol_factor_steps).  sn: IPX_ND_FIELDS int64 per supernode --
 *   0 first position   1 s   2 b   3 offset of its boundary in bnd_rows / cmap / upd
 *   4 offset of its front in `fronts`   5 ld   6 pad   7, 8 its children: child_idx[7 .. 8)
 *   9 offset of its ld + 1 doubles in `work` (large fronts)
 * lists: supernode numbers, a launch takes lists[off .. off + cnt).  perm / bnd_rows: the ROW of
 * A behind an own / a boundary index.  No floating-point atomics, every sum in a fixed order: the
 * same values give the same bits. */
#define IPX_ND_FIELDS 12
typedef struct {
  int64_t m, nsuper;
  const int64_t *sn;
  const int32_t *perm, *bnd_rows, *cmap, *child_idx, *lists;
  const int32_t *A_rowptr, *A_colidx;
  const double *A_val;
  double *fronts, *work, *y, *upd;
  int32_t *flag;
} ipx_nd_args;
int ipx_nd_small_max(void);
/* Small fronts of one level, a workgroup each: the entries of S from the rows of A (merge of two
 * sorted rows, in storage order), the children's updates added through cmap child after child,
 * the partial Cholesky of the s own columns.  flag: bit 0 -- a pivot fell below 2^-43 of its
 * diagonal entry of S; bit 2 (with bit 0) -- a pivot was <= 0.  fmax: the largest front of the
 * list (sizes the LDS).  assemble_only != 0 (either path): the fronts are left as assembled, not
 * factored -- what the tests compare with S. */
int ipx_nd_factor_small(const ipx_nd_args *a, int64_t off, int64_t cnt, int32_t fmax,
                        int32_t assemble_only, void *stream);
/* Large fronts of one level: assembly, the children's updates (one launch per child ordinal),
 * then per front s / 64 (rounded up) tile-column steps.  sn_host: the table `sn` in host memory.
 * Same flag bits. */
int ipx_nd_factor_large(const ipx_nd_args *a, const int64_t *sn_host, const int32_t *lists_host,
                        int64_t off, int64_t cnt, int32_t assemble_only, void *stream);
/* v = (A A')^-1 w in the caller's row order, a launch per level upwards and one downwards, a
 * workgroup per front.  Upwards: x = [w[own rows]; 0] + the children's update vectors (child
 * order), L11 y = x1 -> y[positions], upd[boundary] = x2 - L21 y.  Downwards: L11' x1 = y - L21'
 * x[boundary rows], x[own rows] = x1.  levels_host: per level (offset into lists, number of
 * fronts, the largest front -- it sizes the LDS, at most 4096). */
int ipx_nd_solve(const ipx_nd_args *a, int32_t nlevels, const int64_t *levels_host, const double *w,
                 double *x, void *stream);
/* `steps` tile-column steps of ipx_chol_factor (M a multiple of 64, steps <= M / 64): the
 * leading 64 * steps columns hold L, the rest the Schur complement (lower triangle).  work (M + 1
 * doubles) is the caller's: work[i] the diagonal entry pivot i is judged against, work[M] a
 * running minimum of pivot / entry.  flag is not cleared; bits as ipx_chol_factor's. */
int ipx_chol_factor_steps(int64_t M, double *G, int64_t steps, int *flag, double *work,
                          void *stream);

/* ---- the same factorization in SKIP mode, for a rank-deficient A (ipsolver/nested.py
 * PivotSkippingNestedSolver, ipsolver/sparse_deficient.py).  A pivot d with
 * |d| <= 2^-43 S_kk (S_kk the assembled diagonal entry, the quantity bit 0 compares with; a zero
 * row, S_kk = 0, included) is SKIPPED: row perm[k] of A depends on the rows eliminated before it.
 * Its column of L is zero, its diagonal is stored as +inf, the trailing matrix takes no update, no
 * flag bit is raised and work[M] does not see it.  A pivot d < -2^-43 S_kk, or a NaN, stays bits
 * 0 | 2.  What remains is the factorization of A_S A_S', S the kept rows; ipx_nd_solve on it
 * (unchanged: x / inf = 0) returns (A_S A_S')^-1 w_S on S and exactly 0 on the dropped rows.
 * Arguments, launch shapes and every other convention as the entries without _skip, whose results
 * do not change. */
int ipx_nd_factor_small_skip(const ipx_nd_args *a, int64_t off, int64_t cnt, int32_t fmax,
                             int32_t assemble_only, void *stream);
int ipx_nd_factor_large_skip(const ipx_nd_args *a, const int64_t *sn_host,
                             const int32_t *lists_host, int64_t off, int64_t cnt,
                             int32_t assemble_only, void *stream);
int ipx_chol_factor_steps_skip(int64_t M, double *G, int64_t steps, int *flag, double *work,
                               void *stream);
/* mark[row] = 1 where the stored diagonal of the row's own position is +inf, else 0 (m ints, the
 * caller's row order): one pass over the fronts' diagonals */
int ipx_nd_skipped(const ipx_nd_args *a, int32_t *mark, void *stream);
/* The q dropped rows d_rows (ascending, 0 <= q <= ipx_border_pmax()) beside the q x q Woodbury
 * kernels above; Y column-major m x q with zero rows at the dropped rows.
 * ipx_nd_dropped_fold: t[i] = 0 for a dropped row, else b[i] + sum_j Y[i + m j] b[d_rows[j]]
 * (j ascending).  ipx_nd_dropped_fill (q >= 1): out[i] = u[i] for a kept row,
 * out[d_rows[j]] = sum_g part[g * q + j] over the ipx_border_groups(m) partial blocks of an
 * ipx_border_tdot, g ascending.  One launch each, no atomics. */
int ipx_nd_dropped_fold(int64_t m, int32_t q, const double *Y, const int32_t *d_rows,
                        const int32_t *mark, const double *b, double *t, void *stream);
int ipx_nd_dropped_fill(int64_t m, int32_t q, const double *part, const int32_t *d_rows,
                        const int32_t *mark, const double *u, double *out, void *stream);

/* ---- projected GLTR (csrc/gltr.hip, ipsolver/gltr.py) ----
 * The Lanczos recurrence of the Generalized Lanczos Trust Region method on vectors of n doubles,
 * with the trust-region problem of its tridiagonal T solved on the device after every step.
 * Q: (kmax + 1) columns of n doubles, column j at Q + j n.  State block
 * (ipx_gltr_state_doubles(kmax) doubles, written by ipx_gltr_start):
 *   [0] stop code (0 running, 4 tolerance or invariant subspace, 1 cap), [1] vectors used k,
 *   [2] gamma_0, [3] R, [4] tol, [5] lambda, [6] ||h||, [7] q_T(h) = 1/2 h'T h + gamma_0 h_0,
 *   [8] gamma_{k+1}, [9] case (0 interior, 1 boundary, 2 near-hard), [10] cap,
 *   [11] exit path of the tridiagonal solve (0 interior, 1 secular iteration converged,
 *   2 near-hard, 3 collapsed bracket), [12] its rounds, [13] the last delta, [14..15] spare,
 *   [16...] diag[kmax] (delta_j), off[kmax] (gamma_{j+1}), h[kmax].
 * Every reduction is per-workgroup partials (part: ipx_gltr_part_doubles(n) doubles) folded in a
 * fixed order by the consumer; no atomics.  Host arguments do not change from step to step, so
 * steps are enqueued blind: once the stop code is set every launch of a later step returns at
 * once and leaves state and Q as they are. */
#define IPX_GLTR_MAX_VECTORS 256
int64_t ipx_gltr_state_doubles(int32_t kmax);
int ipx_gltr_grid(int64_t n);
int64_t ipx_gltr_part_doubles(int64_t n);
/* gamma_0 = ||g||, q_0 = g / gamma_0 into column 0, the header (tol < 0: the default
 * max(min(0.01 gamma_0, 0.1 gamma_0^2), 1e-25); gamma_0^2 < tol stops at once with code 4, no
 * vector used); cap <= kmax bounds the vectors.  Two launches. */
int ipx_gltr_start(int64_t n, int32_t kmax, int32_t cap, const double *g, double *Q, double *state,
                   double *part, double radius, double tol, void *stream);
/* one step from w = Z H q_k (k read from the state on the device): delta_k = q_k'w,
 * column k + 1 <- (w - delta_k q_k) - gamma_k q_{k-1} (no gamma term at k = 0), gamma_{k+1} its
 * norm, T extended, h = argmin 1/2 h'T h + gamma_0 h_0 over ||h|| <= R, stop when
 * (gamma_{k+1} h_k)^2 < tol, gamma_{k+1} <= 1e-14 gamma_0 or k + 1 reaches the cap; otherwise
 * column k + 1 /= gamma_{k+1}.  Four launches. */
int ipx_gltr_step(int64_t n, int32_t kmax, const double *w, double *Q, double *state, double *part,
                  void *stream);
/* x[i] = (x0 ? x0[i] : 0) + sum_{j < k} h[j] Q[j n + i], j ascending, separate multiply and add;
 * 16-byte accesses when n is even and Q, x0, x are 16-byte aligned.  One launch. */
int ipx_gltr_combine(int64_t n, int32_t kmax, const double *Q, const double *state,
                     const double *x0, double *x, void *stream);
/* The tridiagonal trust-region solve alone: diag[k], off[k - 1] (> 0), g0 > 0, radius > 0;
 * out[0..5] = lambda, ||h||, q_T(h), case, exit path, rounds, out[8 ... 8 + k) = h.  The host twin
 * runs the same routine with the device's lanes one after the other. */
int ipx_gltr_tridiag(int32_t k, const double *diag, const double *off, double g0, double radius,
                     double *out, void *stream);
int ipx_gltr_tridiag_host(int32_t k, const double *diag, const double *off, double g0,
                          double radius, double *out);

#ifdef __cplusplus
}
#endif
#endif /* IPX_H */
