// Limited-memory quasi-Newton Hessians in compact form (ipsolver/quasi_newton.py):
//
//     B = sigma I + W C W',   W = [S Y]  (n x 2M, column j at W + j n),  C  (2M x 2M)
//
// S and Y are two rings of M columns each; slot t holds the pair (s_t, y_t) in columns t and
// M + t.  Columns of slots never written are zero and so are their rows / columns of C, so
// every product runs over all R = 2M columns.  The state block (ipx_lowrank_state_doubles):
//
//     [0] sigma  [1] stored pairs k  [2] next slot  [3] updates  [4] skipped
//     [5] sigma fixed (LSR1)  [6] the last update was stored  [7] its slot
//     [IPX_LR_HDR ...] the Gram W'W (R x R), then C (R x R)
//
// An update is three launches and no read-back:
//   k_lr_wdot (two rows of the grid)   partials of s'W, y'W, s's, s'y, y'y
//   k_lr_middle (one workgroup)        folds them, applies the skip rule, forms the middle
//                                      matrix from the Gram, inverts it in LDS, rewrites the
//                                      header, the Gram row / column of the slot and C
//   k_lr_commit                        copies s, y into the slot when the pair was stored
// A product is two: partials of W'p, then every workgroup folds them in the same order,
// forms c = C (W'p) and writes out (+)= sigma p + W c.
//
// The middle-matrix arithmetic is one __host__ __device__ routine (lr_middle): the device runs
// it in one workgroup, ipx_lowrank_middle_host runs the same operations in the same order on
// the host, so CPU tests pin the numbers.
//
// At the end of the file: ipx_csr_tdiff_dot, the y of a pair whose memory also approximates
// constraint Hessians -- [g+ - g] + (J(x+) - J(x))' v in one launch per constraint.
#include "ipx_common.h"
#include <math.h>
#include <string.h>

#define LR_RMAX (2 * IPX_LR_MAX_MEMORY)
#define LR_NQMAX (2 * LR_RMAX + 3)
#define LR_GRID_CAP 512

namespace {

// what lr_middle keeps between its phases (LDS on the device, the stack on the host)
struct LrShared {
  double a[LR_RMAX * LR_RMAX];     // the middle matrix, inverted in place
  double d[LR_NQMAX];              // s'W, y'W, s's, s'y, y'y
  double c[LR_RMAX];               // C (W's) for the SR1 test
  double rowmax[LR_RMAX];
  double sig, amax;
  int sl[IPX_LR_MAX_MEMORY];       // chronological index -> slot
  int perm[LR_RMAX];
  int ok, piv;
};

#ifdef __HIP_DEVICE_COMPILE__
#define LR_SYNC() __syncthreads()
#else
#define LR_SYNC() do { } while (0)
#endif

// Gram entry (i, j) with the candidate pair in slot `head` (columns hs = head, hy = M + head)
__host__ __device__ inline double lr_gram(const double *G, const double *d, int R, int hs,
                                          int hy, int i, int j) {
  if (i != hs && i != hy && (j == hs || j == hy)) { const int t = i; i = j; j = t; }
  const double ss = d[2 * R], sy = d[2 * R + 1], yy = d[2 * R + 2];
  if (i == hs) return j == hs ? ss : j == hy ? sy : d[j];
  if (i == hy) return j == hs ? sy : j == hy ? yy : d[R + j];
  return G[(int64_t)i * R + j];
}

// One update of the state block from the folded dot products in S.d.  `tid` / `nt`: this
// thread's share of the parallel loops (the host passes 0 / 1); every reduction a decision
// rests on runs in one thread in a fixed order.
__host__ __device__ inline void lr_middle(LrShared &S, double *st, int kind, int M,
                                          double init_scale, double thresh, int tid, int nt) {
  const int R = 2 * M;
  double *G = st + IPX_LR_HDR, *C = G + (int64_t)R * R;
  const double *d = S.d;
  const double ss = d[2 * R], sy = d[2 * R + 1], yy = d[2 * R + 2];
  if (!(ss != 0.0)) {                    // the same point again: not an update, not counted
    LR_SYNC();
    if (tid == 0) st[6] = 0.0;
    return;
  }
  const int k = (int)st[1], head = (int)st[2];
  const int hs = head, hy = M + head;
  // ---- the skip rule
  if (kind == 0) {
    if (tid == 0) {
      S.ok = sy > thresh * sqrt(ss * yy);
      S.sig = init_scale > 0.0 ? init_scale : yy / sy;
    }
  } else {
    double sig;
    if (st[5] != 0.0) sig = st[0];
    else if (init_scale > 0.0) sig = init_scale;
    else sig = (sy > 0.0 && yy / sy > 0.0) ? yy / sy : 1.0;
    for (int t = tid; t < R; t += nt) {
      double v = 0.0;
      for (int j = 0; j < R; ++j) v += C[(int64_t)t * R + j] * d[j];
      S.c[t] = v;
    }
    LR_SYNC();
    if (tid == 0) {
      double uc = 0.0, yc = 0.0, cgc = 0.0;
      for (int t = 0; t < R; ++t) {
        uc += d[t] * S.c[t];
        yc += d[R + t] * S.c[t];
        double g = 0.0;
        for (int j = 0; j < R; ++j) g += G[(int64_t)t * R + j] * S.c[j];
        cgc += S.c[t] * g;
      }
      const double sbs = sig * ss + uc;                     // s'Bs
      const double ybs = sig * sy + yc;                     // y'Bs
      const double bsbs = ((sig * sig) * ss + (2.0 * sig) * uc) + cgc;   // ||Bs||^2
      const double den = sy - sbs;
      double nr2 = (yy - 2.0 * ybs) + bsbs;                 // ||y - Bs||^2
      if (nr2 < 0.0) nr2 = 0.0;
      S.ok = fabs(den) > 0.0 && fabs(den) >= thresh * sqrt(ss * nr2);
      S.sig = sig;
    }
  }
  LR_SYNC();
  if (!S.ok) {
    LR_SYNC();
    if (tid == 0) { st[4] += 1.0; st[6] = 0.0; }
    return;
  }
  // ---- the middle matrix of the pairs kept with the candidate, in chronological order
  const int kn = k + 1 < M ? k + 1 : M;
  const int K = kind == 0 ? 2 * kn : kn;
  const double sig = S.sig;
  for (int t = tid; t < kn; t += nt) S.sl[t] = (head - kn + 1 + t + M) % M;
  LR_SYNC();
  for (int e = tid; e < K * K; e += nt) {
    const int i = e / K, j = e % K;
    double v;
    if (kind == 0) {                     // [[sigma S'S, L], [L', -D]]
      const int a = i % kn, b = j % kn;
      const int sa = S.sl[a], sb = S.sl[b];
      if (i < kn && j < kn) v = sig * lr_gram(G, d, R, hs, hy, sa, sb);
      else if (i < kn) v = a > b ? lr_gram(G, d, R, hs, hy, sa, M + sb) : 0.0;
      else if (j < kn) v = b > a ? lr_gram(G, d, R, hs, hy, sb, M + sa) : 0.0;
      else v = a == b ? -lr_gram(G, d, R, hs, hy, sa, M + sa) : 0.0;
    } else {                             // D + L + L' - sigma S'S
      const int sa = S.sl[i], sb = S.sl[j];
      const double sty = i >= j ? lr_gram(G, d, R, hs, hy, sa, M + sb)
                                : lr_gram(G, d, R, hs, hy, sb, M + sa);
      v = sty - sig * lr_gram(G, d, R, hs, hy, sa, sb);
    }
    S.a[i * K + j] = v;
  }
  LR_SYNC();
  for (int i = tid; i < K; i += nt) {
    double m = 0.0;
    for (int j = 0; j < K; ++j) m = fmax(m, fabs(S.a[i * K + j]));
    S.rowmax[i] = m;
  }
  LR_SYNC();
  if (tid == 0) {
    double m = 0.0;
    for (int i = 0; i < K; ++i) m = fmax(m, S.rowmax[i]);
    S.amax = m;
    S.ok = 1;
  }
  LR_SYNC();
  // ---- Gauss-Jordan in place with partial pivoting (row swaps undone on the columns at the end)
  for (int p = 0; p < K; ++p) {
    if (tid == 0) {
      int r = p;
      double best = fabs(S.a[p * K + p]);
      for (int i = p + 1; i < K; ++i) {
        const double v = fabs(S.a[i * K + p]);
        if (v > best) { best = v; r = i; }
      }
      S.piv = r;
      S.perm[p] = r;
      if (!(best > 1e-14 * S.amax)) S.ok = 0;
    }
    LR_SYNC();
    if (!S.ok) break;
    const int r = S.piv;
    if (r != p)
      for (int j = tid; j < K; j += nt) {
        const double t = S.a[p * K + j];
        S.a[p * K + j] = S.a[r * K + j];
        S.a[r * K + j] = t;
      }
    LR_SYNC();
    const double piv = S.a[p * K + p];
    LR_SYNC();
    for (int j = tid; j < K; j += nt) S.a[p * K + j] = (j == p ? 1.0 : S.a[p * K + j]) / piv;
    LR_SYNC();
    for (int i = tid; i < K; i += nt) {
      if (i == p) continue;
      const double f = S.a[i * K + p];
      for (int j = 0; j < K; ++j) S.a[i * K + j] = (j == p ? 0.0 : S.a[i * K + j]) - f * S.a[p * K + j];
    }
    LR_SYNC();
  }
  if (!S.ok) {
    LR_SYNC();
    if (tid == 0) { st[4] += 1.0; st[6] = 0.0; }
    return;
  }
  for (int p = K - 1; p >= 0; --p) {
    const int r = S.perm[p];
    if (r != p)
      for (int i = tid; i < K; i += nt) {
        const double t = S.a[i * K + p];
        S.a[i * K + p] = S.a[i * K + r];
        S.a[i * K + r] = t;
      }
    LR_SYNC();
  }
  // ---- commit: the Gram row / column of the slot, C, the header
  for (int j = tid; j < R; j += nt) {
    const double gs = lr_gram(G, d, R, hs, hy, hs, j), gy = lr_gram(G, d, R, hs, hy, hy, j);
    if (j == hs || j == hy) continue;
    G[(int64_t)hs * R + j] = gs; G[(int64_t)j * R + hs] = gs;
    G[(int64_t)hy * R + j] = gy; G[(int64_t)j * R + hy] = gy;
  }
  if (tid == 0) {
    G[(int64_t)hs * R + hs] = ss;
    G[(int64_t)hs * R + hy] = sy;
    G[(int64_t)hy * R + hs] = sy;
    G[(int64_t)hy * R + hy] = yy;
  }
  for (int e = tid; e < R * R; e += nt) C[e] = 0.0;
  LR_SYNC();
  for (int e = tid; e < kn * kn; e += nt) {
    const int a = e / kn, b = e % kn;
    const int sa = S.sl[a], sb = S.sl[b];
    double css, csy, cys, cyy;
    if (kind == 0) {                     // -[sigma S  Y] M^-1 [sigma S  Y]'
      css = -(sig * (sig * S.a[a * K + b]));
      csy = -(sig * S.a[a * K + kn + b]);
      cys = -(sig * S.a[(kn + a) * K + b]);
      cyy = -S.a[(kn + a) * K + kn + b];
    } else {                             // (Y - sigma S) M^-1 (Y - sigma S)'
      const double v = S.a[a * K + b];
      css = sig * (sig * v);
      csy = -(sig * v);
      cys = csy;
      cyy = v;
    }
    C[(int64_t)sa * R + sb] = css;
    C[(int64_t)sa * R + M + sb] = csy;
    C[(int64_t)(M + sa) * R + sb] = cys;
    C[(int64_t)(M + sa) * R + M + sb] = cyy;
  }
  if (tid == 0) {
    st[0] = sig;
    st[1] = (double)kn;
    st[2] = (double)((head + 1) % M);
    st[3] += 1.0;
    st[5] = 1.0;
    st[6] = 1.0;
    st[7] = (double)head;
  }
}

int lr_grid(int64_t n) { return ipx_grid_for(n, IPX_BLOCK * 4, LR_GRID_CAP); }

// Partials of v'W (R sums) per workgroup into part[(q0 + j) G + b]; the two rows of the grid
// take v = s and v = y, the first adds s's and s'y (at q = 2R, 2R + 1), the second y'y (2R + 2).
// v1 == NULL: one row, v = v0, no extras (the product's W'p).
template <int RC>
__global__ void __launch_bounds__(IPX_BLOCK)
k_lr_wdot(int64_t n, int R, const double *__restrict__ W, const double *__restrict__ v0,
          const double *__restrict__ v1, double *__restrict__ part) {
  __shared__ double lds[(RC + 2) * (IPX_BLOCK / IPX_WAVE)];
  const int G = gridDim.x, b = blockIdx.x, row = blockIdx.y;
  const double *v = row ? v1 : v0;
  double acc[RC + 2];
#pragma unroll
  for (int j = 0; j < RC + 2; ++j) acc[j] = 0.0;
  for (int64_t i = (int64_t)b * IPX_BLOCK + threadIdx.x; i < n; i += (int64_t)G * IPX_BLOCK) {
    const double x = v[i];
#pragma unroll
    for (int j = 0; j < RC; ++j)
      if (j < R) acc[j] += x * W[(int64_t)j * n + i];
    if (v1) {
      if (row == 0) { acc[RC] += x * x; acc[RC + 1] += x * v1[i]; }
      else acc[RC] += x * x;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < RC + 2; ++j) {
    const double s = ipx_wave_sum(acc[j]);
    if (lane == 0) lds[j * 4 + wave] = s;
  }
  __syncthreads();
  const int nx = v1 ? (row == 0 ? 2 : 1) : 0;
  for (int q = threadIdx.x; q < R + nx; q += IPX_BLOCK) {
    const int j = q < R ? q : RC + (q - R);
    const double s = ((lds[j * 4] + lds[j * 4 + 1]) + lds[j * 4 + 2]) + lds[j * 4 + 3];
    const int dst = q < R ? row * R + q : 2 * R + row * 2 + (q - R);
    part[(int64_t)dst * G + b] = s;
  }
}

// nq sums of G partials each (part[q G + b]), into out[q]: wave w folds quantities w, w+4, ...,
// lane l adds entries l, l+64, ... in order, then the DPP butterfly -- the same order in every
// workgroup that calls it
__device__ void lr_fold(const double *__restrict__ part, int G, int nq, double *out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int q = wave; q < nq; q += IPX_BLOCK / IPX_WAVE) {
    double v = 0.0;
    for (int b = lane; b < G; b += IPX_WAVE) v += part[(int64_t)q * G + b];
    v = ipx_wave_sum(v);
    if (lane == 0) out[q] = v;
  }
  __syncthreads();
}

__global__ void __launch_bounds__(IPX_BLOCK)
k_lr_middle(int kind, int M, double init_scale, double thresh, const double *__restrict__ part,
            int G, double *st) {
  __shared__ LrShared S;
  lr_fold(part, G, 4 * M + 3, S.d);
  lr_middle(S, st, kind, M, init_scale, thresh, threadIdx.x, IPX_BLOCK);
}

__global__ void __launch_bounds__(IPX_BLOCK)
k_lr_commit(int64_t n, int M, const double *__restrict__ st, const double *__restrict__ s,
            const double *__restrict__ y, double *__restrict__ W) {
  if (st[6] == 0.0) return;
  const int64_t slot = (int64_t)st[7];
  double *ws = W + slot * n, *wy = W + (M + slot) * n;
  for (int64_t i = (int64_t)blockIdx.x * IPX_BLOCK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * IPX_BLOCK) {
    ws[i] = s[i];
    wy[i] = y[i];
  }
}

// out (+)= sigma p + W c, c = C (W'p) from the partials of k_lr_wdot (same grid)
__global__ void __launch_bounds__(IPX_BLOCK)
k_lr_apply(int64_t n, int R, const double *__restrict__ W, const double *__restrict__ st,
           const double *__restrict__ part, const double *__restrict__ p,
           double *__restrict__ out, int accumulate) {
  __shared__ double u[LR_RMAX], c[LR_RMAX];
  lr_fold(part, gridDim.x, R, u);
  const double *C = st + IPX_LR_HDR + (int64_t)R * R;
  for (int t = threadIdx.x; t < R; t += IPX_BLOCK) {
    double v = 0.0;
    for (int j = 0; j < R; ++j) v += C[(int64_t)t * R + j] * u[j];
    c[t] = v;
  }
  __syncthreads();
  const double sigma = st[0];
  for (int64_t i = (int64_t)blockIdx.x * IPX_BLOCK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * IPX_BLOCK) {
    double v = sigma * p[i];
    for (int j = 0; j < R; ++j) v += W[(int64_t)j * n + i] * c[j];
    out[i] = accumulate ? out[i] + v : v;
  }
}

// The CG loop's form of the product (ipx_cg_args.LR_*): Hp (+)= sigma p + W c on rows < rows,
// the base of the other rows kept; p'Hp partials of the final Hp over all n rows into
// part1[G + b] in the H.p kernels' layout.  The same per-row arithmetic as k_lr_apply with
// accumulate (out = base + (sigma p + W c)).  Both kernels of the pair read the loop's stop word
// and return when it is set.
__global__ void __launch_bounds__(IPX_BLOCK)
k_lr_apply_cg(int64_t n, int64_t rows, int R, const double *__restrict__ W,
              const double *__restrict__ st, const double *__restrict__ part,
              const double *__restrict__ p, double *__restrict__ Hp,
              const double *__restrict__ diag, int has_base, double *__restrict__ part1,
              const double *__restrict__ guard) {
  if (guard && *guard != 0.0) return;
  __shared__ double u[LR_RMAX], c[LR_RMAX], red[IPX_BLOCK / IPX_WAVE];
  lr_fold(part, gridDim.x, R, u);
  const double *C = st + IPX_LR_HDR + (int64_t)R * R;
  for (int t = threadIdx.x; t < R; t += IPX_BLOCK) {
    double v = 0.0;
    for (int j = 0; j < R; ++j) v += C[(int64_t)t * R + j] * u[j];
    c[t] = v;
  }
  __syncthreads();
  const double sigma = st[0];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * IPX_BLOCK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * IPX_BLOCK) {
    const double pi = p[i];
    double h = has_base ? Hp[i] : (diag ? diag[i] * pi : 0.0);
    if (i < rows) {
      double v = sigma * pi;
      for (int j = 0; j < R; ++j) v += W[(int64_t)j * rows + i] * c[j];
      h = h + v;
    }
    Hp[i] = h;
    acc += pi * h;
  }
  acc = ipx_block_reduce<IPX_SUM>(acc, red);
  if (threadIdx.x == 0) {
    part1[blockIdx.x] = 0.0;
    part1[gridDim.x + blockIdx.x] = acc;
  }
}

template <int RC>
__global__ void __launch_bounds__(IPX_BLOCK)
k_lr_wdot_guarded(int64_t n, int R, const double *__restrict__ W, const double *__restrict__ v,
                  double *__restrict__ part, const double *__restrict__ guard) {
  if (guard && *guard != 0.0) return;
  __shared__ double lds[RC * (IPX_BLOCK / IPX_WAVE)];
  const int G = gridDim.x, b = blockIdx.x;
  double acc[RC];
#pragma unroll
  for (int j = 0; j < RC; ++j) acc[j] = 0.0;
  for (int64_t i = (int64_t)b * IPX_BLOCK + threadIdx.x; i < n; i += (int64_t)G * IPX_BLOCK) {
    const double x = v[i];
#pragma unroll
    for (int j = 0; j < RC; ++j)
      if (j < R) acc[j] += x * W[(int64_t)j * n + i];
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < RC; ++j) {
    const double s = ipx_wave_sum(acc[j]);
    if (lane == 0) lds[j * 4 + wave] = s;
  }
  __syncthreads();
  for (int q = threadIdx.x; q < R; q += IPX_BLOCK)
    part[(int64_t)q * G + b] = ((lds[q * 4] + lds[q * 4 + 1]) + lds[q * 4 + 2]) + lds[q * 4 + 3];
}

int launch_wdot(int64_t n, int R, const double *W, const double *v0, const double *v1,
                double *part, int G, hipStream_t st) {
  const dim3 grid(G, v1 ? 2 : 1), block(IPX_BLOCK);
  if (R <= 8) hipLaunchKernelGGL(k_lr_wdot<8>, grid, block, 0, st, n, R, W, v0, v1, part);
  else if (R <= 16) hipLaunchKernelGGL(k_lr_wdot<16>, grid, block, 0, st, n, R, W, v0, v1, part);
  else if (R <= 32) hipLaunchKernelGGL(k_lr_wdot<32>, grid, block, 0, st, n, R, W, v0, v1, part);
  else hipLaunchKernelGGL(k_lr_wdot<64>, grid, block, 0, st, n, R, W, v0, v1, part);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

bool lr_args_ok(int64_t n, int32_t mem) {
  return n > 0 && mem >= 1 && mem <= IPX_LR_MAX_MEMORY;
}

}  // namespace

int ipx_lowrank_cg_launch(int64_t n, int64_t rows, int mem, const double *W, const double *state,
                          double *part, const double *p, double *Hp, const double *diag,
                          int has_base, double *part1, const double *guard, hipStream_t st) {
  if (!lr_args_ok(rows, mem) || rows > n || !W || !state || !part || !p || !Hp || !part1)
    return IPX_EINVAL;
  const int G = lr_grid(rows), R = 2 * mem;
  const dim3 grid(G), block(IPX_BLOCK);
  // (the same partial sums as k_lr_wdot's for one vector: the same c, the same bits per row as
  // the operator form's product)
  if (R <= 8) hipLaunchKernelGGL(k_lr_wdot_guarded<8>, grid, block, 0, st, rows, R, W, p, part, guard);
  else if (R <= 16) hipLaunchKernelGGL(k_lr_wdot_guarded<16>, grid, block, 0, st, rows, R, W, p, part, guard);
  else if (R <= 32) hipLaunchKernelGGL(k_lr_wdot_guarded<32>, grid, block, 0, st, rows, R, W, p, part, guard);
  else hipLaunchKernelGGL(k_lr_wdot_guarded<64>, grid, block, 0, st, rows, R, W, p, part, guard);
  IPX_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_lr_apply_cg, grid, block, 0, st, n, rows, R, W, state,
                     (const double *)part, p, Hp, diag, has_base, part1, guard);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

extern "C" {

int64_t ipx_lowrank_state_doubles(int32_t mem) {
  const int64_t R = 2 * (int64_t)mem;
  return IPX_LR_HDR + 2 * R * R;
}

int ipx_lowrank_grid(int64_t n) { return lr_grid(n); }

int64_t ipx_lowrank_part_doubles(int64_t n, int32_t mem) {
  return (4 * (int64_t)mem + 3) * lr_grid(n);
}

int ipx_lowrank_update(int32_t kind, int64_t n, int32_t mem, double init_scale, double threshold,
                       double *W, const double *s, const double *y, double *state, double *part,
                       void *stream) {
  if (!lr_args_ok(n, mem) || (kind != 0 && kind != 1) || !W || !s || !y || !state || !part)
    return IPX_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int G = lr_grid(n), R = 2 * mem;
  int rc = launch_wdot(n, R, W, s, y, part, G, st);
  if (rc) return rc;
  hipLaunchKernelGGL(k_lr_middle, dim3(1), dim3(IPX_BLOCK), 0, st, (int)kind, (int)mem, init_scale,
                     threshold, (const double *)part, G, state);
  IPX_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_lr_commit, dim3(ipx_grid_for(n, IPX_BLOCK * 4)), dim3(IPX_BLOCK), 0, st, n,
                     (int)mem, (const double *)state, s, y, W);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

int ipx_lowrank_apply(int64_t n, int32_t mem, const double *W, const double *state, const double *p,
                      double *out, int32_t accumulate, double *part, void *stream) {
  if (!lr_args_ok(n, mem) || !W || !state || !p || !out || !part || out == p) return IPX_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int G = lr_grid(n), R = 2 * mem;
  int rc = launch_wdot(n, R, W, p, nullptr, part, G, st);
  if (rc) return rc;
  hipLaunchKernelGGL(k_lr_apply, dim3(G), dim3(IPX_BLOCK), 0, st, n, R, W, state,
                     (const double *)part, p, out, (int)accumulate);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

void ipx_lowrank_middle_host(int32_t kind, int32_t mem, double init_scale, double threshold,
                             double *state, const double *dots) {
  if (mem < 1 || mem > IPX_LR_MAX_MEMORY) return;
  static thread_local LrShared S;
  memcpy(S.d, dots, sizeof(double) * (4 * mem + 3));
  lr_middle(S, state, kind, mem, init_scale, threshold, 0, 1);
}

}  // extern "C"

// ---- the pair's y for constraint terms: y (+)= [g+ - g] + (J(x+) - J(x))' v -------------------
//
// One memory approximates the sum of the Lagrangian-Hessian terms declared with a strategy
// (quasi_newton.LagrangianQN), so its y needs (J+ - J)' v of every such constraint.  J+ and J share
// one CSR pattern; the kernel walks the TRANSPOSED pattern (CSRPattern.transpose: row j = column j
// of J, its entries' rows in t_rowidx, their positions in J's value array in t_perm) and reads
// both value arrays through the permutation -- no transposed value array is made.  Row j:
//
//     y[j] = ((accumulate ? y[j] : 0) + (base_new ? base_new[j] - base_old[j] : 0))
//            + sum_k v[t_rowidx[k]] * (val_new[t_perm[k]] - val_old[t_perm[k]])
//
// the sum from 0 in stored order, plain operations (-ffp-contract=off).  The tiles are spmv.hip's:
// a workgroup streams its tile's entries (lane i -> entry i), parks the terms in LDS, then one
// lane per row adds its terms left to right.  A row longer than a tile has a tile of its own:
// the workgroup stages it chunk by chunk and ONE lane carries the sum through the chunks, so every
// row has the host routine's order whatever its length (no atomics, no tree).
//
// Algorithmic HBM bytes: 36 per entry (row index 4, permutation 8, two values 16, the gathered
// v 8) + 4 (n + 1) row pointers + 8 n out (+ 8 n per base vector, + 8 n when accumulating).
namespace {

constexpr int TD_TILE_NNZ = IPX_SPMV_TILE_NNZ;

__host__ __device__ inline double lr_tdiff_mul(double v, double a_new, double a_old) {
  return v * (a_new - a_old);
}

__host__ __device__ inline double lr_tdiff_term(int64_t k, const int32_t *ri, const int64_t *perm,
                                                const double *vn, const double *vo,
                                                const double *v) {
  const int64_t p = perm[k];
  return lr_tdiff_mul(v[ri[k]], vn[p], vo[p]);
}

// sum + the terms [a, b) of a row, left to right; `terms` (staged by the caller: term k at
// terms[k - off]) or, NULL, straight from the arrays
__host__ __device__ inline double lr_tdiff_sum(double sum, int64_t a, int64_t b,
                                               const double *terms, int64_t off,
                                               const int32_t *ri, const int64_t *perm,
                                               const double *vn, const double *vo,
                                               const double *v) {
  for (int64_t k = a; k < b; ++k)
    sum = sum + (terms ? terms[k - off] : lr_tdiff_term(k, ri, perm, vn, vo, v));
  return sum;
}

// the per-row routine: row j of the transposed pattern from its finished sum
__host__ __device__ inline double lr_tdiff_row(int64_t j, double sum, const double *base_new,
                                               const double *base_old, const double *y,
                                               int accumulate) {
  const double head = accumulate ? y[j] : 0.0;
  const double base = base_new ? base_new[j] - base_old[j] : 0.0;
  return (head + base) + sum;
}

__global__ void __launch_bounds__(IPX_BLOCK)
k_csr_tdiff_dot(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ rowidx,
                const int64_t *__restrict__ perm, const int32_t *__restrict__ tiles, int ntiles,
                const double *__restrict__ vn, const double *__restrict__ vo,
                const double *__restrict__ v, const double *__restrict__ base_new,
                const double *__restrict__ base_old, double *y, int accumulate) {
  __shared__ double terms[TD_TILE_NNZ];
  const int tile = ipx_xcd_item(blockIdx.x, ntiles);
  if (tile < 0) return;
  const int r0 = tiles[tile], r1 = tiles[tile + 1];
  const int s = tiles[ntiles + 1 + tile], e = tiles[ntiles + 2 + tile];
  const int tid = threadIdx.x;
  if (e - s <= TD_TILE_NNZ) {
    if (e > s) {
      // every load of a lane issued before the first use: indices, then the three gathers
      constexpr int U = TD_TILE_NNZ / IPX_BLOCK;
      int ri[U];
      int64_t p[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = min(s + tid + u * IPX_BLOCK, e - 1);
        ri[u] = rowidx[k];
        p[u] = perm[k];
      }
      double mv[U], a[U], b[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        mv[u] = v[ri[u]];
        a[u] = vn[p[u]];
        b[u] = vo[p[u]];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = s + tid + u * IPX_BLOCK;
        if (k < e) terms[k - s] = lr_tdiff_mul(mv[u], a[u], b[u]);
      }
    }
    __syncthreads();
    for (int r = r0 + tid; r < r1; r += IPX_BLOCK) {
      const double sum = lr_tdiff_sum(0.0, rowptr[r], rowptr[r + 1], terms, s, nullptr, nullptr,
                                      nullptr, nullptr, nullptr);
      y[r] = lr_tdiff_row(r, sum, base_new, base_old, y, accumulate);
    }
    return;
  }
  // a tile is over-long only when it is a single very long row
  for (int r = r0; r < r1; ++r) {
    const int a = rowptr[r], b = rowptr[r + 1];
    double sum = 0.0;
    for (int c = a; c < b; c += TD_TILE_NNZ) {
      const int ce = min(c + TD_TILE_NNZ, b);
      for (int k = c + tid; k < ce; k += IPX_BLOCK)
        terms[k - c] = lr_tdiff_term(k, rowidx, perm, vn, vo, v);
      __syncthreads();
      if (tid == 0)
        sum = lr_tdiff_sum(sum, c, ce, terms, c, nullptr, nullptr, nullptr, nullptr, nullptr);
      __syncthreads();
    }
    if (tid == 0) y[r] = lr_tdiff_row(r, sum, base_new, base_old, y, accumulate);
  }
}

bool tdiff_args_ok(int64_t n, int64_t m, int64_t nnz, const void *rowptr, const void *rowidx,
                   const void *perm, const void *vn, const void *vo, const void *v,
                   const void *base_new, const void *base_old, const void *y) {
  if (n < 0 || m < 0 || nnz < 0 || nnz > INT32_MAX || n > INT32_MAX || m > INT32_MAX) return false;
  if ((base_new == nullptr) != (base_old == nullptr)) return false;
  if (n > 0 && (!rowptr || !y)) return false;
  if (nnz > 0 && (m == 0 || !rowidx || !perm || !vn || !vo || !v)) return false;
  return true;
}

}  // namespace

extern "C" {

int ipx_csr_tdiff_dot(int64_t n, int64_t m, int64_t nnz, const int32_t *t_rowptr,
                      const int32_t *t_rowidx, const int64_t *t_perm, const int32_t *t_tiles,
                      int32_t t_ntiles, const double *val_new, const double *val_old,
                      const double *v, const double *base_new, const double *base_old, double *y,
                      int32_t accumulate, void *stream) {
  if (!tdiff_args_ok(n, m, nnz, t_rowptr, t_rowidx, t_perm, val_new, val_old, v, base_new,
                     base_old, y) || t_ntiles < 0 || (n > 0 && (!t_tiles || t_ntiles < 1)))
    return IPX_EINVAL;
  if (n == 0) return IPX_OK;
  hipLaunchKernelGGL(k_csr_tdiff_dot, dim3(ipx_xcd_grid(t_ntiles)), dim3(IPX_BLOCK), 0,
                     (hipStream_t)stream, t_rowptr, t_rowidx, t_perm, t_tiles, (int)t_ntiles,
                     val_new, val_old, v, base_new, base_old, y, (int)accumulate);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

int ipx_csr_tdiff_dot_host(int64_t n, int64_t m, int64_t nnz, const int32_t *t_rowptr,
                           const int32_t *t_rowidx, const int64_t *t_perm, const double *val_new,
                           const double *val_old, const double *v, const double *base_new,
                           const double *base_old, double *y, int32_t accumulate) {
  if (!tdiff_args_ok(n, m, nnz, t_rowptr, t_rowidx, t_perm, val_new, val_old, v, base_new,
                     base_old, y))
    return IPX_EINVAL;
  if (n > 0 && (t_rowptr[0] != 0 || t_rowptr[n] != nnz)) return IPX_EINVAL;
  for (int64_t j = 0; j < n; ++j)
    if (t_rowptr[j + 1] < t_rowptr[j]) return IPX_EINVAL;
  for (int64_t k = 0; k < nnz; ++k)
    if (t_rowidx[k] < 0 || t_rowidx[k] >= m || t_perm[k] < 0 || t_perm[k] >= nnz)
      return IPX_EINVAL;
  for (int64_t j = 0; j < n; ++j) {
    const double sum = lr_tdiff_sum(0.0, t_rowptr[j], t_rowptr[j + 1], nullptr, 0, t_rowidx,
                                    t_perm, val_new, val_old, v);
    y[j] = lr_tdiff_row(j, sum, base_new, base_old, y, accumulate);
  }
  return IPX_OK;
}

}  // extern "C"
