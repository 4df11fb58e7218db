// Device-resident projected CG iteration (Steihaug-Toint; reference
// qp_subproblem.py:549-634) for gfx950.
//
// The reference loop has three scalar-gated branches per iteration
// (rt_g < tol :551, p'Hp <= 0 :558, ||x_next|| >= radius :583).  Reading those
// scalars on the host costs more than the HBM time of the whole iteration, so
// here they never leave the device: every kernel's prologue folds the
// per-workgroup partial sums left by its predecessor in a FIXED order (so all
// workgroups derive bit-identical scalars), takes the branch, and workgroup 0
// records it in a small state block.  A non-zero `stop` field turns every
// later kernel of the stream into a no-op; the host reads the state block
// only once per batch of iterations.
//
// One iteration, step by step (general sparsity: one launch each):
//
//   step1  alpha = rt_g / p'Hp;  r += alpha*Hp;  partials of ||x+alpha p||^2,
//          # of box violations of x + alpha p            (x itself untouched)
//   spmv   w = A r
//   banded v = (AA')^-1 w, with ||A g||^2 = ||w - (AA')v||^2 partials from the same
//          launch(es)                                    (orthogonality, projections.py:52)
//   spmv   r = r - A'v  (= g_next; the reference sets r = g, :632), ||g||^2 partials
//   step2  checks: ||x_next|| >= radius -> stop 2; box violated -> stop 5 (host
//          finishes the iteration); orthogonality > tol -> stop 6 (host refines);
//          else beta = ||g||^2/rt_g;  x += alpha p;  p = beta p - g
//   spmv   Hp = H p (+ diag*p), p'Hp partials
//
// For banded problems the steps pair up into THREE launches (same arithmetic):
//   k_cg_step1_ar      step1 inside the A.r SpMV        (banded A, no box)
//   k_solve_decoupled  the banded solve with g = r - A'v as its tail (banded.hip;
//                      tridiagonal A A', separator system numerically diagonal)
//   k_cg_step2_hp      step2 inside the H.p SpMV        (banded H)
// each falling back to the separate launches when its structural condition fails
// (checked symbolically by ipsolver/cg_fused.py).
//
// ... and, beyond the resident kernel's size, into TWO: the first two as k_step1_solve_tail
// (banded.hip; rows of A of one length <= 16, the cyclic-reduction solve).  g then lands in the
// buffer r was not read from: inside a batch r and r_next swap roles by iteration, and
// cg_iterate ends with one guarded copy (k_cg_settle_r) that leaves the current r in a->r.
//
// Because x is only advanced in step2, every early exit leaves (x, p, alpha)
// exactly as the reference's exit paths (:565-576, :585-596) need them.
//
// Host side (behind the kernels):
//   LoopPlan  which form each stage takes for an argument block and how many partials it
//             leaves, derived ONCE per entry-point call (plan_of) and passed down by reference
//   tables    the instantiations of k_cg_step1_box / k_cg_step1_ar / k_cg_step2_hp, each set
//             written out once with the reason beside what is absent
//   halves    launch_projection_half (step1 .. g = r - A'v) and launch_update_half (compaction,
//             step2, H.p, low-rank tail, tile boundaries of p): the batch loop, both forms of
//             the sharded segment, ipx_cg_resume and ipx_cg_step2_hp call them with their own
//             data (HalfArgs).  A new step1 or solve form is a value of the plan's enums and an
//             arm of one half.
#include "ipx_common.h"
#include <algorithm>
#include <vector>

// (state block layout: ipx_common.h ST_*)

namespace {

IPX_STAMP_DECL(ipx_dbg_cg);
#define CG_STAMP(k) IPX_STAMP_TO(ipx_dbg_cg, k)

constexpr int VB = IPX_BLOCK;

constexpr int VU = 8;        // elements per lane per trip, loads issued together (one trip at n = 1e6)

typedef ipx_own_ranges OwnRanges;      // (ipx_common.h)
// kernel argument of the PEER forms: the peer job; an empty struct for the others (the job is
// ~350 bytes of kernel arguments the single-GPU launches should not carry: measured +0.2 us on
// the dominant kernel)
struct ipx_no_peer {};
template <bool PEER> struct peer_arg { typedef ipx_no_peer type; };
template <> struct peer_arg<true> { typedef ipx_peer_job type; };
static OwnRanges own_all(int64_t n) {
  OwnRanges o;
  for (int k = 0; k < 4; ++k) { o.lo[k] = 0; o.hi[k] = 0; }
  o.hi[0] = n;
  return o;
}

__global__ void __launch_bounds__(VB)
k_cg_step1(int64_t n, double *st, int parity, const double *__restrict__ p1, int np1,
           const double *__restrict__ x, const double *__restrict__ p, double *r,
           const double *__restrict__ Hp, const double *__restrict__ lb,
           const double *__restrict__ ub, double *__restrict__ p2, int nchunks, OwnRanges own) {
  // own: the elements that count in ||x + alpha p||^2 and the box test (all of them on one
  // GPU; a rank's own entries in the row-sharded loop, whose halo copies are updated by the
  // same launch)
  __shared__ double lds[VB / IPX_WAVE];
  // chunk c of nchunks: a contiguous run of elements, owned by a fixed XCD
  const int c = ipx_xcd_item(blockIdx.x, nchunks);
  if (c < 0) return;
  const int64_t len = (n + nchunks - 1) / nchunks;
  const int64_t lo_i = (int64_t)c * len, hi_i = min(n, lo_i + len);
  int64_t i0 = lo_i + threadIdx.x;
  // Request order = arrival order (vmcnt counts in order): first the state
  // words and the partials of p'Hp (second half of the SpMV's partials: x.y
  // sums), then the first trip's operands.  The scalar fold below then runs
  // while the operand loads are still streaming in.
  const double *const fparts[1] = {p1 + np1};
  const int fcounts[1] = {np1};
  const double stop = st[ST_STOP];
  const double rtg = st[parity ? ST_RTG1 : ST_RTG0];
  const double tol = st[ST_TOL];
  ipx_fold_regs<1> fold;
  fold.load(fparts, fcounts);
  double xv[VU], pv[VU], rv[VU], hv[VU], lo[VU], hi[VU];
#pragma unroll
  for (int u = 0; u < VU; ++u) {
    const int64_t i = min(i0 + u * VB, n - 1);
    xv[u] = x[i]; pv[u] = p[i]; rv[u] = r[i]; hv[u] = Hp[i];
    if (lb) { lo[u] = lb[i]; hi[u] = ub ? ub[i] : HUGE_VAL; }
  }
  if (stop != 0.0) return;
  const bool lead = c == 0 && threadIdx.x == 0;
  double fout[1];
  fold.finish(fparts, fcounts, lds, fout);
  const double ptHp = fout[0];
  if (rtg < tol) {                                   // qp_subproblem.py:551
    if (lead) st[ST_STOP] = 4.0;
    return;
  }
  if (ptHp <= 0.0) {                                 // :558
    if (lead) { st[ST_NITER] += 1.0; st[ST_PTHP] = ptHp; st[ST_STOP] = 3.0; }
    return;
  }
  const double alpha = rtg / ptHp;                   // :579
  if (lead) { st[ST_NITER] += 1.0; st[ST_PTHP] = ptHp; st[ST_ALPHA] = alpha; }
  double sx = 0.0, viol = 0.0;
  while (true) {
#pragma unroll
    for (int u = 0; u < VU; ++u) {
      const int64_t i = i0 + u * VB;
      if (i < hi_i) {
        const double xn = xv[u] + alpha * pv[u];     // :580 (not stored)
        if (own.has(i)) {
          sx += xn * xn;
          if (lb) viol += ((lo[u] <= xn) && (xn <= hi[u])) ? 0.0 : 1.0;   // :599
        }
        r[i] = rv[u] + alpha * hv[u];                // :622
      }
    }
    i0 += VU * VB;
    if (i0 >= hi_i) break;
#pragma unroll
    for (int u = 0; u < VU; ++u) {
      const int64_t i = min(i0 + u * VB, n - 1);
      xv[u] = x[i]; pv[u] = p[i]; rv[u] = r[i]; hv[u] = Hp[i];
      if (lb) { lo[u] = lb[i]; hi[u] = ub ? ub[i] : HUGE_VAL; }
    }
  }
  const double a = ipx_block_reduce<IPX_SUM>(sx, lds);
  const double b = ipx_block_reduce<IPX_SUM>(viol, lds);
  if (threadIdx.x == 0) { p2[c] = a; p2[nchunks + c] = b; }
}

// step1 for the barrier problem's box-Schur projection (solver_kind 1 with group tables):
// the same updates and sums as k_cg_step1, but the elements are visited group by group
// (shared column + the rows' private columns; then the columns of no group), so that the
// first stage of the projection -- w_S from r_next, t = B^-1 w_S, up = r_next - alpha't
// (csrc/boxschur.hip k_pairs_pre) -- happens on the values just formed instead of in a
// launch of its own that reads r again.  `rounds` items per thread, SB_ITEMS or a few more
// (ipx_balanced_rounds: one partial per 2048+ items).
constexpr int SB_ITEMS = 8;
constexpr int SB_RMIN = 5;       // fewest rounds (part2 holds n / 1024 + 2 entries per half:
                                 // cg_fused.py; 3 rounds are as fast but triple the partials)
// items whose loads are in flight together in the computed-columns form (measured at config 5
// with 8 rounds: 1 -> 22.0, 2 -> 22.3, 4 -> 23.9, 8 -> 36 us: the kernel wants workgroups per CU,
// not loads per lane -- DESIGN.md section 6)
constexpr int SB_BATCH = 1;

// MODE: the form of the group tables (ipx_group_tab: full, compact coefficients, compact
// coefficients + computed columns; the same numbers bit for bit).
// PEER (row-sharded loop on the peer mailboxes): p1 holds zeros for the tiles of halo rows (the
// PEER form of k_cg_step2_hp and ipx_cg_shard2_fold_hp see to that), so its sum is the rank's
// own p'Hp; summed over the ranks here (ipx_peer_sum), unguarded like in k_cg_step1_ar.
template <bool PEER, int MODE>
__global__ void __launch_bounds__(IPX_BLOCK)
k_cg_step1_box(double *st, int parity, const double *__restrict__ p1, int np1,
               const double *__restrict__ x, const double *__restrict__ p, double *__restrict__ r,
               const double *__restrict__ Hp, const double *__restrict__ lb,
               const double *__restrict__ ub, double *__restrict__ p2, int nblk, int ng, int ngen,
               ipx_group_tab T, const int32_t *__restrict__ gen_cols, int ny,
               double *__restrict__ up, OwnRanges own, int rounds,
               typename peer_arg<PEER>::type pj) {
  __shared__ double lds[IPX_BLOCK / IPX_WAVE];
  __shared__ double plds[PEER ? IPX_MAX_PEERS + 1 : 1];
  const int blk = ipx_xcd_item(blockIdx.x, nblk);
  if (blk < 0) return;
  const double *const fparts[1] = {p1 + np1};
  const int fcounts[1] = {np1};
  const double stop = st[ST_STOP];
  const double rtg = st[parity ? ST_RTG1 : ST_RTG0];
  const double tol = st[ST_TOL];
  ipx_fold_regs<1> fold;
  fold.load(fparts, fcounts);
  if (!PEER && stop != 0.0) return;
  if (PEER && stop == 7.0) return;                   // (a mailbox wait timed out: k_cg_step2_hp)
  const bool lead = blk == 0 && threadIdx.x == 0;
  double fout[1];
  fold.finish(fparts, fcounts, lds, fout);
  if constexpr (PEER) {
    double tot[1];
    if (!ipx_peer_sum<1>(pj.pv, pj.seq, 1, fout, blk == 0, plds, tot)) {
      if (threadIdx.x == 0) { st[ST_STOP] = 7.0; st[ST_VIOL] = 4.0 + 10.0 * blk; }
      return;
    }
    fout[0] = tot[0];
    if (stop != 0.0) return;
  }
  const double ptHp = fout[0];
  if (rtg < tol) {                                   // qp_subproblem.py:551
    if (lead) st[ST_STOP] = 4.0;
    return;
  }
  if (ptHp <= 0.0) {                                 // :558
    if (lead) { st[ST_NITER] += 1.0; st[ST_PTHP] = ptHp; st[ST_STOP] = 3.0; }
    return;
  }
  const double alpha = rtg / ptHp;                   // :579
  if (lead) { st[ST_NITER] += 1.0; st[ST_PTHP] = ptHp; st[ST_ALPHA] = alpha; }
  double sx = 0.0, viol = 0.0;
  const int nitems = ng + ngen;
  // one item: the updates of its (up to three) elements and the first stage of the projection
  // (e[t] < 0: no such element); the same expressions whichever way the operands were loaded
  auto item = [&](const int (&e)[3], bool grp, double ap, double sp, double aq, double sq,
                  const double (&xv)[3], const double (&pv)[3], const double (&rv)[3],
                  const double (&hv)[3], const double (&lo)[3], const double (&hi)[3]) {
    double rn[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const double xn = xv[t] + alpha * pv[t];                 // :580 (not stored)
      rn[t] = rv[t] + alpha * hv[t];                           // :622
      if (e[t] >= 0) {
        if (own.has(e[t])) {                                   // (sharded: own entries only)
          sx += xn * xn;
          if (lb) viol += ((lo[t] <= xn) && (xn <= hi[t])) ? 0.0 : 1.0;   // :599
        }
        r[e[t]] = rn[t];
      }
    }
    const int c = e[0];
    if (grp) {
      const int cp = e[1], cq = e[2];
      const double rc = rn[0], rp = cp >= 0 ? rn[1] : 0.0, rq = cq >= 0 ? rn[2] : 0.0;
      const double wp = cp < 0 ? ap * rc : (cp > c ? ap * rc + sp * rp : sp * rp + ap * rc);
      const double wq = cq < 0 ? aq * rc : (cq > c ? aq * rc + sq * rq : sq * rq + aq * rc);
      double i11, i12, i22, wgt, ut;
      ipx_group_inverse(cq != -2, ap, sp, aq, sq, i11, i12, i22, wgt);
      if (cq == -2) {
        ut = ap * (i11 * wp);
      } else {
        const double tp = i11 * wp + i12 * wq;
        const double tq = i12 * wp + i22 * wq;
        ut = ap * tp + aq * tq;
      }
      if (c < ny) up[c] = rc - ut;
    } else if (c < ny) {
      up[c] = rn[0];
    }
  };
  if constexpr (MODE == IPX_GROUPS_AFFINE) {
    // computed columns: nothing depends on a table, so all the loads of an item (SB_BATCH items)
    // are requested at once, indices clamped instead of branches -- with the table forms below
    // every item is a table -> gather round trip
    for (int k0 = 0; k0 < rounds; k0 += SB_BATCH) {
      int e[SB_BATCH][3];
      bool grp[SB_BATCH], valid[SB_BATCH];
      double ep[SB_BATCH], eq[SB_BATCH];
      double xv[SB_BATCH][3], pv[SB_BATCH][3], rv[SB_BATCH][3], hv[SB_BATCH][3];
      double lo[SB_BATCH][3], hi[SB_BATCH][3];
#pragma unroll
      for (int k = 0; k < SB_BATCH; ++k) {
        const int i = (blk * rounds + k0 + k) * IPX_BLOCK + threadIdx.x;
        const bool on = k0 + k < rounds;                      // (uniform)
        valid[k] = on && i < nitems;
        const int ic = min(i, nitems - 1);
        grp[k] = ic < ng;
        const int gi = min(ic, ng - 1);
        const int e0 = grp[k] ? T.c0 + ic : T.gen0 + (ic - ng);
        e[k][0] = e0; e[k][1] = grp[k] ? e0 + T.dp : e0; e[k][2] = grp[k] ? e0 + T.dq : e0;
        if (on) {
          ep[k] = T.grp2[2 * gi]; eq[k] = T.grp2[2 * gi + 1];
#pragma unroll
          for (int t = 0; t < 3; ++t) {
            const int j = e[k][t];
            xv[k][t] = x[j]; pv[k][t] = p[j]; rv[k][t] = r[j]; hv[k][t] = Hp[j];
          }
        } else {
          ep[k] = eq[k] = 0.0;
#pragma unroll
          for (int t = 0; t < 3; ++t) xv[k][t] = pv[k][t] = rv[k][t] = hv[k][t] = 0.0;
        }
      }
      if (lb) {
#pragma unroll
        for (int k = 0; k < SB_BATCH; ++k)
#pragma unroll
          for (int t = 0; t < 3; ++t) lo[k][t] = k0 + k < rounds ? lb[e[k][t]] : 0.0;
      } else {
#pragma unroll
        for (int k = 0; k < SB_BATCH; ++k)
#pragma unroll
          for (int t = 0; t < 3; ++t) lo[k][t] = -HUGE_VAL;
      }
      if (ub) {
#pragma unroll
        for (int k = 0; k < SB_BATCH; ++k)
#pragma unroll
          for (int t = 0; t < 3; ++t) hi[k][t] = k0 + k < rounds ? ub[e[k][t]] : 0.0;
      } else {
#pragma unroll
        for (int k = 0; k < SB_BATCH; ++k)
#pragma unroll
          for (int t = 0; t < 3; ++t) hi[k][t] = HUGE_VAL;
      }
#pragma unroll
      for (int k = 0; k < SB_BATCH; ++k) {
        if (!valid[k]) continue;
        const int el[3] = {e[k][0], grp[k] ? e[k][1] : -1, grp[k] ? e[k][2] : -1};
        item(el, grp[k], copysign(1.0, ep[k]), fabs(ep[k]), copysign(1.0, eq[k]), fabs(eq[k]),
             xv[k], pv[k], rv[k], hv[k], lo[k], hi[k]);
      }
    }
  } else {
#pragma unroll 2
    for (int k = 0; k < rounds; ++k) {
      const int i = (blk * rounds + k) * IPX_BLOCK + threadIdx.x;
      if (i >= nitems) continue;
      // every load of the item is requested before the first use: the tables, then the (up
      // to three) elements' x, p, r, Hp and bounds
      const bool grp = i < ng;
      int e[3];
      double ap = 0.0, sp = 0.0, aq = 0.0, sq = 0.0;
      if (grp) {
        ipx_group_cols<MODE>(T, i, e[0], e[1], e[2]);
        ipx_group_coeffs<MODE != IPX_GROUPS_FULL>(T, i, ap, sp, aq, sq);
      } else {
        e[0] = gen_cols[i - ng]; e[1] = -1; e[2] = -1;
      }
      double xv[3], pv[3], rv[3], hv[3], lo[3], hi[3];
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const int j = e[t] >= 0 ? e[t] : e[0];
        xv[t] = x[j]; pv[t] = p[j]; rv[t] = r[j]; hv[t] = Hp[j];
        lo[t] = lb ? lb[j] : -HUGE_VAL;
        hi[t] = ub ? ub[j] : HUGE_VAL;
      }
      item(e, grp, ap, sp, aq, sq, xv, pv, rv, hv, lo, hi);
    }
  }
  const double a = ipx_block_reduce<IPX_SUM>(sx, lds);
  const double b = ipx_block_reduce<IPX_SUM>(viol, lds);
  if (threadIdx.x == 0) { p2[blk] = a; p2[nblk + blk] = b; }
}

// mode bit0: skip the radius / box checks (host already handled them)
//      bit1: skip the orthogonality check (host already refined)
__global__ void __launch_bounds__(VB)
k_cg_step2(int64_t n, double *st, int parity, int mode, const double *__restrict__ p2, int np2,
           const double *__restrict__ p3, int np3, const double *__restrict__ p4, int np4,
           double *x, double *p, const double *__restrict__ g, int nchunks) {
  __shared__ double lds[4 * (VB / IPX_WAVE)];
  CG_STAMP(0);
  const int c = ipx_xcd_item(blockIdx.x, nchunks);   // same element -> XCD map as step1
  if (c < 0) return;
  const int64_t len = (n + nchunks - 1) / nchunks;
  const int64_t lo_i = (int64_t)c * len, hi_i = min(n, lo_i + len);
  int64_t i0 = lo_i + threadIdx.x;
  // Request order = arrival order: state words and the four partial arrays
  // (||x+ap||^2, #violations, ||g||^2, ||A g||^2) first, operands after, so the
  // fold runs while the operands stream in.
  const double *const parts[4] = {p2, p2 + np2, p3, p4};
  const int counts[4] = {(mode & 1) ? 0 : np2, (mode & 1) ? 0 : np2, np3, (mode & 2) ? 0 : np4};
  const double stop = st[ST_STOP];
  const double radius = st[ST_RADIUS], orth_rhs = st[ST_ORTH_RHS];
  const double rtg = st[parity ? ST_RTG1 : ST_RTG0];
  const double alpha = st[ST_ALPHA];
  ipx_fold_regs<4> fold;
  fold.load(parts, counts);
  double xv[VU], pv[VU], gv[VU];
#pragma unroll
  for (int u = 0; u < VU; ++u) {
    const int64_t i = min(i0 + u * VB, n - 1);
    xv[u] = x[i]; pv[u] = p[i]; gv[u] = g[i];
  }
  if (stop != 0.0) return;
  CG_STAMP(1);
  const bool lead = c == 0 && threadIdx.x == 0;
  double red[4];
  fold.finish(parts, counts, lds, red);
  CG_STAMP(2);
  if (!(mode & 1)) {
    const double xn2 = red[0], viol = red[1];
    if (sqrt(xn2) >= radius) {                       // :583
      if (lead) { st[ST_XNORM2] = xn2; st[ST_STOP] = 2.0; }
      return;
    }
    if (viol > 0.0) {                                // :599-616 continues on the host
      if (lead) { st[ST_VIOL] = viol; st[ST_STOP] = 5.0; }
      return;
    }
  }
  const double gg = red[2];                          // ||g_next||^2
  if (!(mode & 2)) {
    const double tt = red[3];                        // ||A g_next||^2
    const double rhs = orth_rhs;
    // orthogonality(A, g) > orth_tol  <=>  ||A g|| > orth_tol ||A||_F ||g||
    if (rhs > 0.0 && gg > 0.0 && sqrt(tt) > rhs * sqrt(gg)) {
      if (lead) { st[ST_ORTH] = sqrt(tt) / sqrt(gg); st[ST_STOP] = 6.0; }
      return;
    }
  }
  const double beta = gg / rtg;                      // :627
  if (lead) {
    st[parity ? ST_RTG0 : ST_RTG1] = gg;             // :633
    st[ST_BETA] = beta;
    st[ST_IT_DONE] += 1.0;
  }
  while (true) {
#pragma unroll
    for (int u = 0; u < VU; ++u) {
      const int64_t i = i0 + u * VB;
      if (i < hi_i) {
        x[i] = xv[u] + alpha * pv[u];                // :580,630
        p[i] = beta * pv[u] - gv[u];                 // :628
      }
    }
    i0 += VU * VB;
    if (i0 >= hi_i) break;
#pragma unroll
    for (int u = 0; u < VU; ++u) {
      const int64_t i = min(i0 + u * VB, n - 1);
      xv[u] = x[i]; pv[u] = p[i]; gv[u] = g[i];
    }
  }
  CG_STAMP(3);
}

// ---- step2 fused into the H.p SpMV (banded Hessians) ------------------------
// step2 rewrites p (and x) element by element and the SpMV right behind it reads
// p back; for a Hessian whose row tiles touch only a few columns outside
// their own row range (halo <= hmax on either side: every banded H) the two
// are one kernel: a workgroup forms p_next = beta p - g on its row range plus
// halo in LDS, stores its own part of p_next and x_next, and takes the SpMV's
// gathers out of LDS.  The halo entries of p are owned (and overwritten in
// place) by the neighbouring workgroups, so their OLD values come from `pb`:
// every tile's first/last hmax entries of p, saved by the kernel that produced
// p (double buffered by iteration parity).  Same expressions in the same
// order as k_cg_step2 + k_csr_spmv: bit-identical results.
// (halo <= 64 and <= the shortest tile: checked by the host binding, cg_fused.fuse_halo)
constexpr int FT_NNZ = IPX_SPMV_TILE_NNZ;

// Carried sums for the radius test (ipx_cg_args.xsums; BOX = false, PEER = false only): what
// k_cg_step2_hp of iteration `it` writes and, with mode bit 4, reads.
//   raw  != NULL: the block's base.  write: the tile's partials of sum x_next^2, x_next p_next,
//        p_next^2 go to raw[q * ntiles + tile] and the lead lane tags them it + 1; !write: x
//        and p change without them, the lead lane clears the tag.
//   in (mode bit 4): the folded sums from the fused step1 + A.r kernel of this iteration, three
//        arrays XS_STRIDE apart (zeros behind their <= XS_STRIDE entries) -- lane t of the
//        workgroup takes entry t of each with the three loads it would spend on the
//        ||x + alpha p||^2 partials, in the same straight-line prologue (a branch there splits
//        the block the fold's loads and the tile's loads are scheduled in: measured +1.5 us).
//        That kernel has compared the raw partials' tag with `it` and left NaNs where they
//        are not this iteration's.
//   The GUARD instantiation (mode bit 8; raw != NULL, write = 0, no mode bit 4) takes the radius
//        guard's X, Q, T (ipx_cg_args.rguard) in `in`, and writes them: the test of :583 is
//        !(T < radius) on the bound the projection half of this iteration left; a launch that
//        commits moves X <- T, Q <- (beta Q + sqrt(gg))(1 + 2^-20) and clears the tag of the
//        sums it does not renew.  (No field of its own: this struct is part of the argument
//        segment of EVERY instantiation -- a word more moves their hidden arguments, for this
//        kernel into another 64-byte line of the segment)
struct ipx_xsums_job {
  double *raw;
  const double *in;
  int it, write;
};
constexpr int XS_SLICE = IPX_XS_SLICE;     // raw partials per folded sum (one wave of k_cg_step1_ar)
constexpr int XS_STRIDE = IPX_XS_STRIDE;   // distance of the three arrays of folded sums
constexpr double XS_BAND = 1e-9; // the carried form decides :583 only outside this relative band

// C16: the column indices come as 16-bit offsets into the tile's span (col - c_lo, built once
// per pattern by the host binding) and the row pointers of a tile whose rows all have the
// same length are not read at all (rowlen[tile] >= 0): 2 + 4/rowlen bytes less per nonzero of
// the 12 a CSR entry costs -- 10 of the 96 MB this kernel moves at n = 1e6.
// A tile whose entry k of row i sits at span offset col16[s] + i + k (every interior tile of a
// banded Hessian) carries ROWLEN_SHIFTED in its rowlen[] word (cg_fused.flagged_rowlen): the GUARD
// form then reads col16[s] alone and forms the other offsets -- the table's 2 bytes per nonzero
// less.  Every other form masks the flag and reads the table (plain and XSUM measured slower
// with the offsets formed: DESIGN.md section 6; BOX and PEER were not tried).
// PEER (row-sharded loop on the peer mailboxes, one segment): p2 / p3 / p4 are the rank's OWN
// ranges of the partial arrays; every workgroup folds them, workgroup 0 sends the four sums to
// the peers and every workgroup adds up the ranks' contributions in rank order (ipx_peer_sum)
// -- the all-reduce of qp_subproblem.py:583,599,626 without a launch of its own.  The halo of
// g travels in the same prologue: two early workgroups store the rank's first / last own
// entries into the neighbours' mailboxes, the tiles whose span reaches into the rank's halo
// take those entries from the mailbox (and write them into g, whose halo the next iteration's
// step1 reads).
// XSUM: the instantiation that writes and / or consumes the carried sums of the radius test
// (ipx_xsums_job).  The launcher picks it only for launches that do; every other launch -- the
// trust_radius = inf loop, the stand-alone entry, BOX, PEER -- runs the kernel without them.
// GUARD: the radius guard's instantiation -- the kernel of the trust_radius = inf loop (no
// ||x + alpha p||^2 partials, no sums; a two-way block sum, gg and tt) that decides :583 from the
// bound T every workgroup loads with its state words (xs.in: the guard's three words).  Without
// mode bit 1 a bound that is not below the radius stops the batch (IPX_CG_STOP_GUARD_LOST); with
// it (a resumed iteration whose test was taken) the bounds advance all the same.
constexpr int ROWLEN_SHIFTED = 1 << 16;      // cg_fused.ROWLEN_SHIFTED (row lengths lie below it)

constexpr int SHIFT_MAX_RL = 8;              // longest row the kernel forms offsets for

// the span offsets of a lane's entries in a flagged tile of RL-entry rows; c[u] comes in as
// the tile's first offset
template <int RL, int U>
__device__ __forceinline__ void shifted_offsets(int (&c)[U], int tid, int last) {
  static_assert(RL >= 1 && RL <= SHIFT_MAX_RL, "a case of the switch in k_cg_step2_hp");
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const unsigned d = (unsigned)min(tid + u * IPX_BLOCK, last);
    c[u] += (int)(d - (RL - 1) * (d / RL));
  }
}

template <bool HAS_DIAG, int Q, int QS, bool BOX, bool C16, bool PEER, bool XSUM = false,
          bool GUARD = false>
__global__ void __launch_bounds__(IPX_BLOCK)
k_cg_step2_hp(int n, double *st, int parity, int mode, const double *__restrict__ p2, int np2,
              const double *__restrict__ p3, int np3, const double *__restrict__ p4, int np4,
              double *x, double *p, const double *__restrict__ g,
              const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
              const double *__restrict__ val, const int32_t *__restrict__ tiles, int ntiles,
              const double *__restrict__ diag, double *__restrict__ Hp,
              double *__restrict__ partial, int hmax, const double *__restrict__ pb_in,
              double *__restrict__ pb_out,
              const uint16_t *__restrict__ col16, const int32_t *__restrict__ rowlen,
              typename peer_arg<PEER>::type pj, double *g_halo, ipx_xsums_job xs) {
  constexpr bool XS = XSUM;                    // the carried sums of the radius test
  constexpr bool SHIFT = C16 && GUARD;         // flagged tiles form their column offsets
  static_assert(!XSUM || (!BOX && !PEER), "carried sums: no box, one GPU");
  static_assert(!GUARD || (!BOX && !PEER && !XSUM), "radius guard: no box, one GPU, no sums");
  // (the folded sums ride in the three loads per lane of the xn2 partials: ipx_fold_regs<2, 3>)
  static_assert(XS_STRIDE == IPX_BLOCK, "one folded entry per lane and load");
  __shared__ double prod[FT_NNZ];
  __shared__ double span[QS * IPX_BLOCK];
  __shared__ int rp[Q * IPX_BLOCK + 1];
  __shared__ double lds[(XSUM ? 5 : 4) * (IPX_BLOCK / IPX_WAVE)];
  __shared__ double plds[PEER ? 4 * IPX_MAX_PEERS + 1 : 1];
  CG_STAMP(0);
  const int tile = ipx_xcd_item(blockIdx.x, ntiles);
  if (tile < 0) return;
  const int tid = threadIdx.x;
  // request order = arrival order: state words and partials first (the fold
  // runs while the operands stream in), then the tile's data
  // (register budget: the partial arrays get as many in-flight loads as their usual
  // lengths need -- step1's <= 512, the SpMV's ~n/1024, the solve's ~m/260 -- not 4 each)
  // BOX = false (no bounds): the violation counts are all zero and are not read; the
  // ||x + alpha p||^2 partials -- one per row tile of A when step1 is fused -- get the
  // freed register instead
  // (mode bit 4: the folded carried sums take the place of the ||x + alpha p||^2 partials --
  // load u of this lane is its entry of array u)
  const bool carried = XS && (mode & 4) != 0;
  const double *const partsA[2] = {BOX ? p2 + np2 : (carried ? xs.in : p2), p4};
  const int countsA[2] = {(GUARD || (mode & 1)) ? 0 : (carried ? 3 * XS_STRIDE : np2),
                          (mode & 2) ? 0 : np4};
  const double *const partsB[1] = {p3};
  const int countsB[1] = {np3};
  const double *const partsC[1] = {BOX ? p2 : p2 + np2};     // BOX: xn2;  else unused (count 0)
  const int countsC[1] = {(BOX && !(mode & 1)) ? np2 : 0};
  const double stop = st[ST_STOP];
  const double radius = st[ST_RADIUS], orth_rhs = st[ST_ORTH_RHS];
  const double rtg = st[parity ? ST_RTG1 : ST_RTG0];
  const double alpha = st[ST_ALPHA];
  double rgT = 0.0, rgQ = 0.0;                 // GUARD: the bound on ||x + alpha p||; Q (lead lane)
  if constexpr (GUARD) {
    rgT = xs.in[IPX_RG_T];
    if (tile == 0 && tid == 0) rgQ = xs.in[IPX_RG_Q];
  }
  ipx_fold_regs<2, BOX ? 2 : 3> foldA;         // BOX: {viol, tt}      else {xn2, tt}
  ipx_fold_regs<1, 4> foldB;                   // gg
  ipx_fold_regs<1, BOX ? 2 : 1> foldC;         // BOX: xn2
  foldA.load(partsA, countsA);
  foldB.load(partsB, countsB);
  if (BOX) foldC.load(partsC, countsC);
  const int r0 = tiles[tile], r1 = tiles[tile + 1];
  const int s = tiles[ntiles + 1 + tile], e = tiles[ntiles + 2 + tile];
  // (requested with the tile's bounds, ahead of the value loads: one wait for all of them)
  const int rlf = C16 ? rowlen[tile] : -1;
  const int rl = rlf < 0 ? -1 : rlf & (ROWLEN_SHIFTED - 1);   // >= 0: every row of the tile has rl entries
  const int nrows = r1 - r0;
  const int c_lo = max(r0 - hmax, 0), c_hi = min(r1 + hmax, n);
  const int nspan = c_hi - c_lo;
  // Q / QS: row / span elements per lane, sized by the launcher from the longest tile
  constexpr int U = FT_NNZ / IPX_BLOCK;
  int c[U];
  double v[U];
  // a flagged tile (cg_fused.shifted_tiles_np; never empty) with a row length phase 1 has a
  // case for: every offset load of the workgroup takes the tile's FIRST offset -- one line, no
  // table traffic -- and phase 1 adds the entry's own part.  (Loads at a selected address, not a
  // branch around them: the prologue stays one block, and it measured 0.02-0.18 us shorter.)
  const bool formed = SHIFT && rlf >= ROWLEN_SHIFTED && rl <= SHIFT_MAX_RL;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int jj = min(s + tid + u * IPX_BLOCK, max(e - 1, 0));   // empty tile: any valid entry
    c[u] = C16 ? (int)col16[formed ? s : jj] : colidx[jj] - c_lo;
    v[u] = val[jj];
  }
  // span operands: element j of the span is column c_lo + j
  double sp[QS], sg[QS];
  const double *pbl = pb_in + (int64_t)(tile - 1) * 2 * hmax + hmax;   // right part of tile-1
  const double *pbr = pb_in + (int64_t)(tile + 1) * 2 * hmax;          // left part of tile+1
#pragma unroll
  for (int k = 0; k < QS; ++k) {
    const int j = min(tid + k * IPX_BLOCK, nspan - 1);
    const int col = c_lo + j;
    sg[k] = g[col];
    // one unconditional load through a selected address (a predicated load would
    // cost a branch and a full wait): left halo = last hmax entries of the previous
    // tile, right halo = first hmax entries of the next one, else p itself
    const double *src = col < r0 ? pbl + (col - (r0 - hmax)) : (col >= r1 ? pbr + (col - r1) : p + col);
    sp[k] = *src;
  }
  // (PEER: the collectives below run even when the loop has stopped -- like the pack kernels
  // they replace -- so that every rank's stores find their readers whatever a workgroup that
  // starts late reads in the stop word: the lead workgroup of THIS launch may have set it).
  // Except after a mailbox wait has timed out (code 7: a peer is gone or cannot run -- two ranks
  // sharing one GPU that is full of the other's spinning workgroups): every later launch of
  // the batch would wait out the 3 s again; the batch is void, the host gives up the transport
  if (!PEER && stop != 0.0) return;
  if (PEER && stop == 7.0) return;
  CG_STAMP(1);
  const bool lead = tile == 0 && tid == 0;
  double red[5], loc[5];
  {
    double la[2], lb1[1], lc[1] = {0.0};
    foldA.local(partsA, countsA, la);
    foldB.local(partsB, countsB, lb1);
    if (BOX) foldC.local(partsC, countsC, lc);
    loc[0] = BOX ? lc[0] : la[0];                  // xn2      (k_cg_step2's order:
    loc[1] = BOX ? la[0] : 0.0;                    // viol      xn2, viol, gg, tt)
    loc[2] = lb1[0];                               // gg
    loc[3] = la[1];                                // tt
    // carried: XX in xn2's place, XP in the (no box: unused) violation count's, PP behind
    // them (selects, one barrier pair as before)
    if constexpr (XS) {
      loc[0] = carried ? foldA.t[0][0] : loc[0];
      loc[1] = carried ? foldA.t[0][1] : loc[1];
      loc[4] = carried ? foldA.t[0][2] : 0.0;
    }
  }
  if constexpr (XS) {
    ipx_block_sum_multi<5>(loc, lds, red);
  } else if constexpr (GUARD) {
    // neither xn2 nor a violation count is formed or read: gg and tt alone go through the block
    // sum (ipx_block_sum_multi sums every component by itself -- the lanes of a wave, then the
    // waves in wave order -- so their bits do not depend on how many travel together)
    double l2[2] = {loc[2], loc[3]}, r2[2];
    ipx_block_sum_multi<2>(l2, lds, r2);
    red[0] = red[1] = red[4] = 0.0;
    red[2] = r2[0];
    red[3] = r2[1];
  } else {
    double l4[4] = {loc[0], loc[1], loc[2], loc[3]}, r4[4];
    ipx_block_sum_multi<4>(l4, lds, r4);
#pragma unroll
    for (int q = 0; q < 4; ++q) red[q] = r4[q];
    red[4] = 0.0;
  }
  if constexpr (PEER) {
    const ipx_peer_view &pv = pj.pv;
    const int par = pj.hseq & 1;
    // push: the rank's first / last own entries of g go to the neighbours' halo areas, by
    // two of the FIRST workgroups dispatched (not by the tiles that own those entries: with
    // more workgroups than the chip holds at once the last tiles start only after the first
    // ones have finished, and the first ones wait for the left neighbour's last entries -- a
    // chain through all the ranks)
    if (tile == min(1, ntiles - 1) && pv.rank > 0)
      for (int k = 0; k < pj.nseg; ++k)
        for (int j = tid; j < pj.send_left[k]; j += IPX_BLOCK)
          ipx_ll_store(pv.mbox[pv.rank - 1] + ipx_peer_halo_word(pv.cap, 1, par, pj.push_l[k] + j),
                       g[pj.own_lo[k] + j], pj.hseq);
    if (tile == min(2, ntiles - 1) && pv.rank < pv.world - 1)
      for (int k = 0; k < pj.nseg; ++k)
        for (int j = tid; j < pj.send_right[k]; j += IPX_BLOCK)
          ipx_ll_store(pv.mbox[pv.rank + 1] + ipx_peer_halo_word(pv.cap, 0, par, pj.push_r[k] + j),
                       g[pj.own_hi[k] - pj.send_right[k] + j], pj.hseq);
    double tot[4], red4[4] = {red[0], red[1], red[2], red[3]};
    bool ok = ipx_peer_sum<4>(pv, pj.seq, 0, red4, tile == 0, plds, tot);
#pragma unroll
    for (int q = 0; q < 4; ++q) red[q] = tot[q];
    // (where the launch-per-collective form leaves them: the host's event handlers and the
    // resumed step2 read the reduced sums there)
    if (lead && pj.pack_out) {
#pragma unroll
      for (int q = 0; q < 4; ++q) pj.pack_out[q] = tot[q];
    }
    // pull: span entries inside the rank's halo come from the neighbours
    const long long deadline = (long long)wall_clock64() + pv.timeout_ticks;
    const unsigned long long *mine = pv.mbox[pv.rank];
    bool okh = true;
#pragma unroll
    for (int k = 0; k < QS; ++k) {
      const int col = c_lo + tid + k * IPX_BLOCK;
      if (tid + k * IPX_BLOCK < nspan) {
        const int64_t word = pj.pull_word(col, par);
        if (word >= 0) {
          double v = 0.0;
          okh = ipx_ll_load(mine + word, pj.hseq, v, deadline) && okh;
          sg[k] = v;
          if (col >= r0 && col < r1) g_halo[col] = v;
        }
      }
    }
    if (!okh) plds[4 * IPX_MAX_PEERS] = 1.0;         // (reset by ipx_peer_sum, read below)
    ipx_lds_barrier();
    const bool okh_all = plds[4 * IPX_MAX_PEERS] == 0.0;
    if (!ok || !okh_all) {                           // a peer died: stop code 7, every rank alike
      // (ST_VIOL: which wait -- 1 the sums, 2 the halo -- and on which tile)
      if (tid == 0) { st[ST_STOP] = 7.0; st[ST_VIOL] = (ok ? 2.0 : 1.0) + 10.0 * tile; }
      return;
    }
    if (stop != 0.0) return;
  }
  if constexpr (GUARD) {
    // :583 from the bound: ||x + alpha p|| <= T < radius -- the test is false.  Anything else
    // (NaN and inf included) decides nothing here
    if (!(mode & 1) && !(rgT < radius)) {
      if (lead) st[ST_STOP] = (double)IPX_CG_STOP_GUARD_LOST;
      return;
    }
  }
  if (!GUARD && !(mode & 1)) {
    double xn2 = red[0], viol = red[1];
    if (carried) {
      // ||x + alpha p||^2 from the sums over the x and p this iteration started from.  M bounds
      // the terms that went into it, so the band covers their cancellation too.  Inside the
      // band, or with sums that are not this iteration's (NaNs: k_cg_step1_ar), the host forms
      // the norm (stop code 10, nothing committed).  radius^2 = +inf (radius 1e300, inf) lies
      // outside the band of every finite M; a non-finite M or value decides nothing.
      const double XX = red[0], XP = red[1], PP = red[4];
      const double a2 = alpha * alpha, r2 = radius * radius;
      xn2 = (XX + 2.0 * (alpha * XP)) + a2 * PP;
      const double M = (XX + 2.0 * fabs(alpha * XP)) + a2 * PP;
      if (!(fabs(xn2 - r2) > XS_BAND * M)) {
        if (lead) st[ST_STOP] = (double)IPX_CG_STOP_RADIUS_UNDECIDED;
        return;
      }
      viol = 0.0;
    }
    if (sqrt(xn2) >= radius) {                       // :583
      if (lead) { st[ST_XNORM2] = xn2; st[ST_STOP] = 2.0; }
      return;
    }
    if (viol > 0.0) {                                // :599-616 continues on the host
      if (lead) { st[ST_VIOL] = viol; st[ST_STOP] = 5.0; }
      return;
    }
  }
  const double gg = red[2];                          // ||g_next||^2
  if (!(mode & 2)) {
    const double tt = red[3];                        // ||A g_next||^2
    if (orth_rhs > 0.0 && gg > 0.0 && sqrt(tt) > orth_rhs * sqrt(gg)) {
      if (lead) { st[ST_ORTH] = sqrt(tt) / sqrt(gg); st[ST_STOP] = 6.0; }
      return;
    }
  }
  CG_STAMP(2);
  const double beta = gg / rtg;                      // :627
  if (lead) {
    st[parity ? ST_RTG0 : ST_RTG1] = gg;             // :633
    st[ST_BETA] = beta;
    st[ST_IT_DONE] += 1.0;
    // x and p change below: tag the sums this launch leaves, or void those it does not renew
    if constexpr (XS) xs.raw[3 * ntiles] = xs.write ? (double)(xs.it + 1) : 0.0;
    if constexpr (GUARD) {
      // (no other workgroup of this launch reads X or Q; T was loaded before any store)
      double *rg = const_cast<double *>(xs.in);
      rg[IPX_RG_Q] = ipx_rguard::step_q(rgQ, beta, gg);
      rg[IPX_RG_X] = rgT;
      xs.raw[3 * ntiles] = 0.0;
    }
  }
  // p_next on the span (LDS), x_next / p_next / boundary copies on the own rows
  double *pbo = pb_out + (int64_t)tile * 2 * hmax;
#pragma unroll
  for (int k = 0; k < QS; ++k) {
    const int j = tid + k * IPX_BLOCK;
    if (j < nspan) {
      const int col = c_lo + j;
      const double pn = beta * sp[k] - sg[k];        // :628
      span[j] = pn;
      if (col >= r0 && col < r1) {
        p[col] = pn;
        if (col - r0 < hmax) pbo[col - r0] = pn;
        if (r1 - col <= hmax) pbo[hmax + (col - (r1 - hmax))] = pn;
      }
    }
  }
  // row pointers, x and the diagonal entries of this lane's rows: requested only now (their registers
  // are not held while the bulk loads are in flight), landed by the time they are needed
  double sx[QS];
#pragma unroll
  for (int k = 0; k < QS; ++k) sx[k] = x[min(max(c_lo + tid + k * IPX_BLOCK, r0), r1 - 1)];
  double dg[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q)
    dg[q] = HAS_DIAG ? diag[r0 + min(tid + q * IPX_BLOCK, nrows - 1)] : 0.0;
  // a tile whose rows all have rl entries: row i's products are prod[i rl .. i rl + rl), no
  // row pointers, in memory or in LDS (a workgroup-uniform test, behind the prologue's loads)
  const bool uniform = C16 && rl >= 0;
  int rpv[Q + 1];
  if (!uniform) {
#pragma unroll
    for (int q = 0; q <= Q; ++q) rpv[q] = rowptr[r0 + min(tid + q * IPX_BLOCK, nrows)] - s;
  }
  CG_STAMP(3);
  ipx_lds_barrier();
  CG_STAMP(4);
  // SpMV phase 1: products with the gathers served from the span.  No test per entry: a lane
  // beyond the tile's entries holds the tile's last one (the clamp of the loads) and leaves its
  // product in a slot of prod[] that phase 2 does not read -- U gathers in flight, not U
  // predicated round trips.  prod[] has a slot for every lane and u (the assert), and phase 2
  // reads slots below e - s only: an irregular tile through rp[] <= e - s, a uniform one up to
  // nrows rl, which is e - s by the way rowlen[] is made (cg_fused.compact_columns: rl >= 0 only
  // where every row of the tile has rl entries).  (An empty tile holds another tile's entry:
  // its column is not this span's.)
  static_assert(U * IPX_BLOCK == FT_NNZ, "one slot of prod[] per lane and product");
  if constexpr (SHIFT) {
    // entry d = i rl + k of a flagged tile sits at span offset col16[s] + i + k =
    // c0 + d - (rl - 1)(d / rl): rl is the workgroup's, the divisors are constants
    if (formed) {
      const int last = e - 1 - s;
      switch (rl) {
        case 1: shifted_offsets<1>(c, tid, last); break;
        case 2: shifted_offsets<2>(c, tid, last); break;
        case 3: shifted_offsets<3>(c, tid, last); break;
        case 4: shifted_offsets<4>(c, tid, last); break;
        case 5: shifted_offsets<5>(c, tid, last); break;
        case 6: shifted_offsets<6>(c, tid, last); break;
        case 7: shifted_offsets<7>(c, tid, last); break;
        default: shifted_offsets<8>(c, tid, last); break;
      }
    }
  }
  if (e > s) {
#pragma unroll
    for (int u = 0; u < U; ++u) prod[tid + u * IPX_BLOCK] = v[u] * span[c[u]];
  }
  if (!uniform) {
#pragma unroll
    for (int q = 0; q <= Q; ++q) {
      const int i = tid + q * IPX_BLOCK;
      if (i <= nrows) rp[i] = rpv[q];
    }
  }
  ipx_lds_barrier();
  CG_STAMP(5);
  // phase 2: row sums, diagonal term, partials of y'y and p'y
  double acc_yy = 0.0, acc_xy = 0.0, yq[Q], sums[Q];
  if (uniform) {
    // entry k of the lane's Q rows together (a lane beyond the tile's rows sums the last row's,
    // for nobody): one trip count for the workgroup, Q reads in flight
    const double *pq[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      pq[q] = prod + min(tid + q * IPX_BLOCK, max(nrows - 1, 0)) * rl;
      sums[q] = 0.0;
    }
#pragma unroll 1
    for (int k = 0; k < rl; ++k) {
#pragma unroll
      for (int q = 0; q < Q; ++q) sums[q] += pq[q][k];
    }
  } else {
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int i = tid + q * IPX_BLOCK;
      double sum = 0.0;
      if (i < nrows) {
        const int a = rp[i], b = rp[i + 1];
        for (int k = a; k < b; ++k) sum += prod[k];
      }
      sums[q] = sum;
    }
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int i = tid + q * IPX_BLOCK;
    yq[q] = 0.0;
    if (i < nrows) {
      const double sum = sums[q];
      const double xr = span[r0 - c_lo + i];
      double y = 1.0 * sum;
      if (HAS_DIAG) y += dg[q] * xr;
      yq[q] = y;
      acc_yy += y * y;
      acc_xy += xr * y;
    }
  }
  CG_STAMP(6);
  const bool xs_out = XS && xs.write != 0;
  double acc_xx = 0.0, acc_xp = 0.0, acc_pp = 0.0;
  // x_next on own span element k of this lane (x was requested before the SpMV phases and has
  // landed); false: not an own row
  auto x_next = [&](int k, double &xn) {
    const int col = c_lo + tid + k * IPX_BLOCK;
    xn = sx[k] + alpha * sp[k];                      // :580,630
    return col >= r0 && col < r1;
  };
  // the sums the next iteration's radius test is formed from: x_next = x + alpha p on the own
  // rows (x was requested before the SpMV phases and has landed) and p_next (still in the span)
  if (xs_out) {
#pragma unroll
    for (int k = 0; k < QS; ++k) {
      double xn;
      if (x_next(k, xn)) {
        const double pn = span[tid + k * IPX_BLOCK];
        acc_xx += xn * xn;
        acc_xp += xn * pn;
        acc_pp += pn * pn;
      }
    }
  }
  if (xs_out) {
    double red5[5] = {acc_yy, acc_xy, acc_xx, acc_xp, acc_pp}, out5[5];
    ipx_block_sum_multi<5>(red5, lds, out5);
    if (tid == 0) {
      partial[tile] = out5[0];
      partial[ntiles + tile] = out5[1];
      xs.raw[tile] = out5[2];
      xs.raw[ntiles + tile] = out5[3];
      xs.raw[2 * ntiles + tile] = out5[4];
    }
  } else {
    double red2[2] = {acc_yy, acc_xy}, out2[2];
    ipx_block_sum_multi<2>(red2, lds, out2);
    // (PEER: the tiles of halo rows leave zeros, so that the consumer may fold the whole array
    // for the rank's own sum -- the barrier problem's own rows are up to four ranges)
    bool counts = true;
    if constexpr (PEER) counts = pj.owns_rows(r0, r1);
    if (tid == 0) {
      partial[tile] = counts ? out2[0] : 0.0;
      partial[ntiles + tile] = counts ? out2[1] : 0.0;
    }
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int i = tid + q * IPX_BLOCK;
    if (i < nrows) Hp[r0 + i] = yq[q];
  }
#pragma unroll
  for (int k = 0; k < QS; ++k) {
    double xn;
    if (x_next(k, xn)) x[c_lo + tid + k * IPX_BLOCK] = xn;
  }
  CG_STAMP(7);
}

// ---- step1 fused into the A.r SpMV (banded Jacobians, no box) ----------------
// step1 rewrites r element by element and the SpMV right behind it reads r
// back.  When the row tiles of A sweep the columns monotonically (every banded
// A) the columns are dealt to the tiles -- tile t owns [own[t], own[t+1]) -- and
// a workgroup forms r_next = r + alpha Hp on its own columns plus the few
// columns beyond them that its rows still touch, in LDS, stores its own part
// and takes the SpMV's gathers out of LDS.  r_next goes to a second buffer
// (the columns beyond the own range belong to the next tile, which must still
// see the old r); the r - A'v SpMV that follows reads it and writes g back into
// r, so outside the iteration nothing changes.  Same expressions in the same
// order as k_cg_step1 + k_csr_spmv; the ||x + alpha p||^2 partials are per tile
// instead of per vector chunk (same values up to the order of summation).
// XN = 1 (NOXN2): trust radius +inf -- ||x + alpha p||^2 can only feed a comparison that is
// always false (:583) and is not formed: x and p are not read at all (16 of the 56 MB this
// kernel moves at n = 1e6).
// XN = 2: the lean form for a FINITE radius.  The test is formed from the sums k_cg_step2_hp of
// the previous iteration left (ipx_cg_args.xsums): x and p are not read either and no part2 is
// written.  Instead the first ncomp workgroups fold one XS_SLICE-entry slice of the three raw
// arrays each (one wave, fixed order), so that every workgroup of the consuming k_cg_step2_hp
// folds 3 x ncomp entries, not 3 x H_ntiles.  They compare the raw partials' tag with `it` and
// pass NaNs on when the sums are not this iteration's.
// XN = 3: the radius guard.  As XN = 1 (no x, no p, no fold, no part2); xs_comp is the guard's
// three words (ipx_cg_args.rguard: X, Q, T) and the lead lane, once it has alpha, stores
// T = (X + |alpha| Q)(1 + 2^-20) for k_cg_step2_hp<.., GUARD> of this iteration.
// C16: column indices as 16-bit offsets into the tile's span (col - own[tile]; the host
// binding builds them once per pattern), 2 bytes instead of 4 per nonzero.
// PEER: p1 is the rank's own range of the p'Hp partials; summed over the ranks in the prologue
// (ipx_peer_sum: workgroup 0 sends, every workgroup adds the contributions in rank order).
template <int QS, int TN, int XN, bool C16, bool PEER>
__global__ void __launch_bounds__(IPX_BLOCK)
k_cg_step1_ar(int n, double *st, int parity, const double *__restrict__ p1, int np1,
              const double *__restrict__ x, const double *__restrict__ p,
              const double *__restrict__ r, double *__restrict__ r_next,
              const double *__restrict__ Hp, const int32_t *__restrict__ rowptr,
              const int32_t *__restrict__ colidx, const double *__restrict__ val,
              const int32_t *__restrict__ tiles, int ntiles, const int32_t *__restrict__ own,
              double *__restrict__ w, double *__restrict__ part2,
              const uint16_t *__restrict__ col16, typename peer_arg<PEER>::type pj,
              const double *__restrict__ xs_raw, int nraw, double *__restrict__ xs_comp,
              int ncomp, int it) {
  constexpr bool NOXN2 = XN != 0;
  __shared__ double prod[TN];
  __shared__ double span[QS * IPX_BLOCK];
  __shared__ int rp[IPX_SPMV_TILE_ROWS + 1];
  __shared__ double lds[IPX_BLOCK / IPX_WAVE];
  __shared__ double plds[PEER ? IPX_MAX_PEERS + 1 : 1];
  CG_STAMP(8);
  const int tile = ipx_xcd_item(blockIdx.x, ntiles);
  if (tile < 0) return;
  const int tid = threadIdx.x;
  const double *const fparts[1] = {p1 + np1};
  const int fcounts[1] = {np1};
  const double stop = st[ST_STOP];
  const double rtg = st[parity ? ST_RTG1 : ST_RTG0];
  const double tol = st[ST_TOL];
  ipx_fold_regs<1, 6> fold;                      // p'Hp partials: one per row tile of H
  fold.load(fparts, fcounts);
  const int r0 = tiles[tile], r1 = tiles[tile + 1];
  const int s = tiles[ntiles + 1 + tile], e = tiles[ntiles + 2 + tile];
  const int nrows = r1 - r0;
  const int o0 = own[tile], o1 = own[tile + 1];          // own columns
  const int c_hi = own[ntiles + 1 + tile];               // one past the last column touched (>= o1)
  const int nspan = c_hi - o0;
  constexpr int U = TN / IPX_BLOCK;
  int c[U];
  double v[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int jj = min(s + tid + u * IPX_BLOCK, max(e - 1, 0));   // empty tile: any valid entry
    c[u] = C16 ? (int)col16[jj] : colidx[jj] - o0;
    v[u] = val[jj];
  }
  double sr[QS], sh[QS], sxv[QS], spv[QS];
#pragma unroll
  for (int k = 0; k < QS; ++k) {
    // (a tile without nonzeros owns nothing: nspan = 0, the clamps keep its loads in range)
    const int col = min(o0 + max(min(tid + k * IPX_BLOCK, nspan - 1), 0), n - 1);
    sr[k] = r[col];
    sh[k] = Hp[col];
    sxv[k] = NOXN2 ? 0.0 : x[col];
    spv[k] = NOXN2 ? 0.0 : p[col];
  }
  // XN = 2: this workgroup's slice of the carried sums' raw partials, one entry per lane of
  // the first wave and array (tile < ncomp <= ceil(nraw / XS_SLICE): the slice is not empty)
  double xq[3] = {0.0, 0.0, 0.0}, xtag = 0.0;
  const bool folds = XN == 2 && tile < ncomp && tid < XS_SLICE;
  if (folds) {
    const int i = tile * XS_SLICE + tid;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const double ld = xs_raw[q * nraw + min(i, nraw - 1)];
      xq[q] = i < nraw ? ld : 0.0;
    }
    xtag = xs_raw[3 * nraw];
  }
  double rgX = 0.0, rgQ = 0.0;                       // XN = 3: the guard's X and Q (lead lane)
  if constexpr (XN == 3) {
    if (tile == 0 && tid == 0) { rgX = xs_comp[IPX_RG_X]; rgQ = xs_comp[IPX_RG_Q]; }
  }
  if (!PEER && stop != 0.0) return;                  // (PEER: see k_cg_step2_hp)
  if (PEER && stop == 7.0) return;
  CG_STAMP(9);
  const bool lead = tile == 0 && tid == 0;
  if (folds) {                                       // (wave-uniform: tid < 64)
#pragma unroll
    for (int q = 0; q < 3; ++q) xq[q] = ipx_wave_sum(xq[q]);
    // sums that are not this iteration's (tag != it) go on as NaNs: the consumer then decides
    // nothing (stop code 10)
    const bool mine = xtag == (double)it;
    if (tid == 0) {
#pragma unroll
      for (int q = 0; q < 3; ++q) xs_comp[q * XS_STRIDE + tile] = mine ? xq[q] : __builtin_nan("");
    }
  }
  double fout[1];
  fold.finish(fparts, fcounts, lds, fout);
  if constexpr (PEER) {
    double tot[1];
    if (!ipx_peer_sum<1>(pj.pv, pj.seq, 1, fout, tile == 0, plds, tot)) {
      if (tid == 0) { st[ST_STOP] = 7.0; st[ST_VIOL] = 3.0 + 10.0 * tile; }
      return;
    }
    fout[0] = tot[0];
    if (stop != 0.0) return;
  }
  const double ptHp = fout[0];
  if (rtg < tol) {                                   // qp_subproblem.py:551
    if (lead) st[ST_STOP] = 4.0;
    return;
  }
  if (ptHp <= 0.0) {                                 // :558
    if (lead) { st[ST_NITER] += 1.0; st[ST_PTHP] = ptHp; st[ST_STOP] = 3.0; }
    return;
  }
  CG_STAMP(10);
  const double alpha = rtg / ptHp;                   // :579
  if (lead) { st[ST_NITER] += 1.0; st[ST_PTHP] = ptHp; st[ST_ALPHA] = alpha; }
  if constexpr (XN == 3) {
    if (lead) xs_comp[IPX_RG_T] = ipx_rguard::step_x(rgX, rgQ, alpha);
  }
  double sx = 0.0;
#pragma unroll
  for (int k = 0; k < QS; ++k) {
    const int j = tid + k * IPX_BLOCK;
    if (j < nspan) {
      const double rn = sr[k] + alpha * sh[k];       // :622
      span[j] = rn;
      if (o0 + j < o1) {                             // own column
        if (!NOXN2) {
          const double xn = sxv[k] + alpha * spv[k]; // :580 (not stored)
          sx += xn * xn;
        }
        r_next[o0 + j] = rn;
      }
    }
  }
  int rpv[(IPX_SPMV_TILE_ROWS / IPX_BLOCK) + 1];
#pragma unroll
  for (int q = 0; q <= IPX_SPMV_TILE_ROWS / IPX_BLOCK; ++q)
    rpv[q] = rowptr[r0 + min(tid + q * IPX_BLOCK, nrows)] - s;
  CG_STAMP(11);
  ipx_lds_barrier();
  CG_STAMP(12);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int jj = s + tid + u * IPX_BLOCK;
    if (jj < e) prod[jj - s] = v[u] * span[c[u]];
  }
#pragma unroll
  for (int q = 0; q <= IPX_SPMV_TILE_ROWS / IPX_BLOCK; ++q) {
    const int i = tid + q * IPX_BLOCK;
    if (i <= nrows) rp[i] = rpv[q];
  }
  ipx_lds_barrier();
  double yq[IPX_SPMV_TILE_ROWS / IPX_BLOCK];
#pragma unroll
  for (int q = 0; q < IPX_SPMV_TILE_ROWS / IPX_BLOCK; ++q) {
    const int i = tid + q * IPX_BLOCK;
    yq[q] = 0.0;
    if (i < nrows) {
      const int a = rp[i], b = rp[i + 1];
      double sum = 0.0;
      for (int k = a; k < b; ++k) sum += prod[k];
      yq[q] = 1.0 * sum;
    }
  }
  CG_STAMP(13);
  if (!NOXN2) {
    const double tot = ipx_block_reduce<IPX_SUM>(sx, lds);
    if (tid == 0) { part2[tile] = tot; part2[ntiles + tile] = 0.0; }
  }
#pragma unroll
  for (int q = 0; q < IPX_SPMV_TILE_ROWS / IPX_BLOCK; ++q) {
    const int i = tid + q * IPX_BLOCK;
    if (i < nrows) w[r0 + i] = yq[q];
  }
  CG_STAMP(14);
}

// Large problems: the per-tile partial arrays grow with n while every consumer
// workgroup folds all of them, so beyond ~1000 entries they are first compacted
// to one entry per 1024 (fixed order: deterministic).  Up to three arrays per
// launch; array k takes blocks [first[k], first[k+1]): its half h, chunk c is
// block first[k] + h*G[k] + c.
struct CompactJob {
  const double *in[3];
  double *out[3];
  int count[3], halves[3], G[3], first[4];
};
__global__ void __launch_bounds__(IPX_BLOCK)
k_compact_partials(CompactJob job, const double *__restrict__ guard) {
  __shared__ double lds[IPX_BLOCK / IPX_WAVE];
  if (guard && *guard != 0.0) return;
  int k = 0;
  while (k < 2 && (int)blockIdx.x >= job.first[k + 1]) ++k;
  const int b = blockIdx.x - job.first[k];
  const int half = b / job.G[k], chunk = b - half * job.G[k];
  const int lo = chunk * 1024, len = min(1024, job.count[k] - lo);
  const double v = ipx_sum_partials<IPX_SUM>(job.in[k] + (int64_t)half * job.count[k] + lo, len, lds);
  if (threadIdx.x == 0) job.out[k][half * job.G[k] + chunk] = v;
}

// First / last hmax entries of p for every row tile of H (both parities): what
// k_cg_step2_hp reads as its halo.  Launched by the unfused producers of p -- who leave no
// carried sums for the radius test: xs_tag (ipx_cg_args.xsums' tag, or NULL) is cleared.
__global__ void __launch_bounds__(IPX_BLOCK)
k_cg_save_pb(const double *__restrict__ p, const int32_t *__restrict__ tiles, int ntiles,
             int hmax, double *__restrict__ pb, double *__restrict__ xs_tag) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx == 0 && xs_tag) *xs_tag = 0.0;
  if (idx >= ntiles * 2 * hmax) return;
  const int t = idx / (2 * hmax), j = idx - t * 2 * hmax;
  const int r0 = tiles[t], r1 = tiles[t + 1];
  const double v = j < hmax ? p[r0 + j] : p[r1 - hmax + (j - hmax)];
  pb[idx] = v;
  pb[(int64_t)ntiles * 2 * hmax + idx] = v;
}

// PJ_STEP1_SOLVE_TAIL: r <- r_next when the batch's last projection left the current r there
// (*where != 0; every workgroup reads the word, nobody writes it: the next batch's first launch
// clears it).
__global__ void __launch_bounds__(VB)
k_cg_settle_r(int64_t n, const int32_t *__restrict__ where, const double *__restrict__ src,
              double *__restrict__ dst) {
  if (*where == 0) return;
  for (int64_t i = (int64_t)blockIdx.x * VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB)
    dst[i] = src[i];
}

// Voids the tag of the carried sums (ipx_cg_args.xsums) on the stream.
__global__ void k_xsums_void(double *xs_tag) { *xs_tag = 0.0; }

// The radius guard behind an update half that ran as the vector step2 (ipx_cg_resume: the test
// of :583 was taken and passed before the host's event): when that launch committed (the stop
// word the caller cleared is still 0) X <- T, Q <- (beta Q + sqrt(gg))(1 + 2^-20) with the beta
// and the ||g_next||^2 it left in the state block.
__global__ void k_rguard_advance(const double *__restrict__ st, int parity, double *rg) {
  if (st[ST_STOP] != 0.0) return;
  const double gg = st[parity ? ST_RTG0 : ST_RTG1];
  rg[IPX_RG_Q] = ipx_rguard::step_q(rg[IPX_RG_Q], st[ST_BETA], gg);
  rg[IPX_RG_X] = rg[IPX_RG_T];
}

// Losing the radius guard (ipx_cg_guard_resume): sum x^2, sum x p, sum p^2 over the current x
// and p into the carried sums' three folded arrays (ipx_xsums_job.in), one entry per workgroup
// and array -- XS_STRIDE workgroups, each over its own run of the vectors, lanes strided within
// it, the block sum in its fixed order: the same bits on every run.  The order differs from the
// per-tile one of k_cg_step2_hp; the band of XS_BAND x M around radius^2 covers that.
__global__ void __launch_bounds__(IPX_BLOCK)
k_rguard_sums(int64_t n, const double *__restrict__ x, const double *__restrict__ p,
              double *__restrict__ comp) {
  __shared__ double lds[3 * (IPX_BLOCK / IPX_WAVE)];
  const int64_t per = (n + XS_STRIDE - 1) / XS_STRIDE;
  const int64_t lo = min((int64_t)blockIdx.x * per, n), hi = min(lo + per, n);
  double acc[3] = {0.0, 0.0, 0.0}, out[3];
  for (int64_t i = lo + threadIdx.x; i < hi; i += IPX_BLOCK) {
    const double xv = x[i], pv = p[i];
    acc[0] += xv * xv;
    acc[1] += xv * pv;
    acc[2] += pv * pv;
  }
  ipx_block_sum_multi<3>(acc, lds, out);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < 3; ++q) comp[q * XS_STRIDE + blockIdx.x] = out[q];
  }
}

// Partitioned row-sharded loop (ipsolver/sharded.py): up to four sub-ranges of partial
// arrays -- the entries produced by a rank's OWN tiles / workgroups -- summed in a fixed
// order into out[0..4): the rank's contribution to an all-reduce.
struct RangeJob {
  const double *ptr[4][4];   // [piece][quantity]; readable even where the count is 0
  int count[4][4];
  int npieces;
  int active;                // bit q: out[q] is written
};

__global__ void __launch_bounds__(256)
k_cg_range_pack(RangeJob job, double *__restrict__ out, const double *__restrict__ guard) {
  __shared__ double lds[4 * 4];
  if (guard && *guard != 0.0) return;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int pc = 0; pc < job.npieces; ++pc) {          // one piece per segment, in order
    double red[4];
    ipx_sum_partials_multi<4>(job.ptr[pc], job.count[pc], lds, red);
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] += red[q];
  }
  if (threadIdx.x < 4 && ((job.active >> threadIdx.x) & 1)) out[threadIdx.x] = acc[threadIdx.x];
}

// The same own-range sums, all-reduced over the ranks INSIDE the kernel (peer mailboxes,
// csrc/peer.hip): workgroup 0 adds up the rank's partials, stores the sums as LL words into
// every rank's mailbox (its own included), waits for the W contributions to its own mailbox
// and adds them in rank order -- every rank derives the same bits -- into out[q].  The other
// workgroups (when a halo plan is given) move the halo of g the same way: the first / last own
// entries of every segment go to the neighbours' mailboxes, the neighbours' arrive in this
// rank's and are copied into the halo entries of g.  Everything a later kernel of this rank
// reads (out, g) is written by this kernel to local memory: no fences, no flags beyond the
// sequence numbers inside the LL words.  A wait that times out (a peer died) raises stop code
// 7 in the state block.
struct HaloPlan {
  int nseg;                                   // 0: no halo exchange in this launch
  int seg_lo[4], own_lo[4], own_hi[4], seg_hi[4], send_left[4], send_right[4];
};

__global__ void __launch_bounds__(256)
k_cg_pack_comm(RangeJob job, double *__restrict__ out, ipx_peer_view pv, uint32_t seq,
               HaloPlan hp, double *__restrict__ g, uint32_t hseq, double *__restrict__ st) {
  __shared__ double lds[4 * 4];
  __shared__ double vals[IPX_MAX_PEERS * 4];
  const int tid = threadIdx.x;
  if (st[ST_STOP] == 7.0) return;        // an earlier wait timed out: do not wait it out again
  const long long deadline = (long long)wall_clock64() + pv.timeout_ticks;
  if (blockIdx.x == 0) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int pc = 0; pc < job.npieces; ++pc) {          // one piece per segment, in order
      double red[4];
      ipx_sum_partials_multi<4>(job.ptr[pc], job.count[pc], lds, red);
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] += red[q];
    }
    const int slot = seq & (IPX_PEER_SLOTS - 1);
    if (tid < 4 * pv.world) {
      const int r = tid >> 2, q = tid & 3;
      if ((job.active >> q) & 1) {
        const double mine = q == 0 ? acc[0] : (q == 1 ? acc[1] : (q == 2 ? acc[2] : acc[3]));
        ipx_ll_store(pv.mbox[r] + ipx_peer_scal_word(slot, pv.rank, q), mine, seq);
      }
    }
    bool ok = true;
    if (tid < 4 * pv.world) {
      const int r = tid >> 2, q = tid & 3;
      double v = 0.0;
      if ((job.active >> q) & 1)
        ok = ipx_ll_load(pv.mbox[pv.rank] + ipx_peer_scal_word(slot, r, q), seq, v, deadline);
      vals[tid] = v;
    }
    if (!ok) st[ST_STOP] = 7.0;
    __syncthreads();
    if (tid < 4 && ((job.active >> tid) & 1)) {
      double s = 0.0;
      for (int r = 0; r < pv.world; ++r) s += vals[4 * r + tid];        // rank order
      out[tid] = s;
    }
    return;
  }
  // ---- halo of g
  const int par = hseq & 1;
  const int nth = (gridDim.x - 1) * blockDim.x, me = (blockIdx.x - 1) * blockDim.x + tid;
  int64_t offL = 0, offR = 0;                   // cumulative counts towards the left / right neighbour
  for (int k = 0; k < hp.nseg; ++k) {
    if (pv.rank > 0)
      for (int j = me; j < hp.send_left[k]; j += nth)       // my first own entries: the left
        ipx_ll_store(pv.mbox[pv.rank - 1] + ipx_peer_halo_word(pv.cap, 1, par, offL + j),   // neighbour's right halo
                     g[hp.own_lo[k] + j], hseq);
    if (pv.rank < pv.world - 1)
      for (int j = me; j < hp.send_right[k]; j += nth)      // my last own entries: the right
        ipx_ll_store(pv.mbox[pv.rank + 1] + ipx_peer_halo_word(pv.cap, 0, par, offR + j),   // neighbour's left halo
                     g[hp.own_hi[k] - hp.send_right[k] + j], hseq);
    offL += hp.send_left[k];
    offR += hp.send_right[k];
  }
  bool ok = true;
  offL = offR = 0;
  const unsigned long long *mine = pv.mbox[pv.rank];
  for (int k = 0; k < hp.nseg; ++k) {
    const int nl = hp.own_lo[k] - hp.seg_lo[k], nr = hp.seg_hi[k] - hp.own_hi[k];
    if (pv.rank > 0)
      for (int j = me; j < nl; j += nth) {
        double v = 0.0;
        ok = ipx_ll_load(mine + ipx_peer_halo_word(pv.cap, 0, par, offL + j), hseq, v, deadline) && ok;
        g[hp.seg_lo[k] + j] = v;
      }
    if (pv.rank < pv.world - 1)
      for (int j = me; j < nr; j += nth) {
        double v = 0.0;
        ok = ipx_ll_load(mine + ipx_peer_halo_word(pv.cap, 1, par, offR + j), hseq, v, deadline) && ok;
        g[hp.own_hi[k] + j] = v;
      }
    offL += nl;
    offR += nr;
  }
  if (!ok) st[ST_STOP] = 7.0;
}

// ================================ host side ================================================
// (structure: see the head of this file)

// step1: k_cg_step1 | k_cg_step1_box, the front of the box-Schur projection | k_cg_step1_ar,
// step1 inside the A.r SpMV (banded A, no box)
enum Step1Form { S1_VECTOR, S1_BOX, S1_FUSED_AR };
// projection: m = 0, g = r | box-Schur, the box rows never multiplied as matrix rows | banded
// solve with g = r - A'v as its tail (one launch) | banded or box-Schur solve, then the A' SpMV |
// dense matvecs w = A r, v = G^-1 w, g = r - A'v, t = A g | step1, w = A r_next, the banded
// solve and its tail as one launch on the solve's windows (csrc/banded.hip k_step1_solve_tail:
// step1 stays S1_FUSED_AR, whose radius modes it takes over, but launches nothing of its own)
enum ProjForm { PJ_NONE, PJ_BOX, PJ_SOLVE_TAIL, PJ_SOLVE_SPMV, PJ_DENSE, PJ_STEP1_SOLVE_TAIL };
// step2: k_cg_step2, then H.p | k_cg_step2_hp, step2 inside the H.p SpMV (banded H)
enum Step2Form { S2_VECTOR, S2_FUSED_HP };
// H.p: the caller's, between the iterations | a low-rank term (+ diagonal) alone | row-major
// n x n in H_val | CSR
enum HpForm { HP_OPERATOR, HP_LOWRANK, HP_DENSE, HP_CSR };

struct LoopPlan {
  Step1Form step1;
  ProjForm proj;
  Step2Form step2;
  HpForm hp;
  bool fused_hp;        // the block enables k_cg_step2_hp (the dense loop still runs the vector step2)
  bool lowrank_tail;    // a low-rank term rides behind the dense / CSR H.p (csrc/lowrank.hip)
  bool no_xn2;          // radius +inf and no box: ||x + alpha p||^2 is neither formed nor folded
  // the radius test of this block's iterations can be formed from the carried sums
  // (ipx_cg_args.xsums): both fused kernels (fused step1 implies no box), a finite radius, and
  // enough workgroups in the fused step1 to fold the raw partials
  bool xsums;
  // ... and is decided from the radius guard's bound instead (ipx_cg_args.rguard, radius_guard):
  // the launches of no_xn2 with the guard's forms of the two fused kernels; the carried sums
  // stay bound for the iteration that loses the guard (ipx_cg_guard_resume)
  bool guard;
  int xs_ncomp;         // folded entries per carried sum: one per XS_SLICE row tiles of H
  // entries per half of part1 .. part4:
  int np1;              // row tiles of a CSR Hessian / workgroups of the dense or low-rank product
  int np2;              // row tiles of A (fused step1), blocks of k_cg_step1_box, or vector chunks
  int np3;              // row tiles of A', or workgroups of whatever forms g with its solve
  int np4;              // workgroups of the solve's residual (||A g||^2)
};

// workgroups of a dense matvec (csrc/dense.hip): rows / 4, capped
int dense_grid(int64_t rows) { return (int)std::min<int64_t>((rows + 3) / 4, 2048); }

int step1_box_rounds(const ipx_boxschur_args *b) {
  return ipx_balanced_rounds(b->ng + b->ngen, SB_RMIN, 2 * SB_ITEMS);
}

LoopPlan plan_of(const ipx_cg_args *a) {
  LoopPlan P{};
  const bool dense = a->solver_kind == 2;
  const bool lowrank = a->LR_W != nullptr && !a->H_operator;
  P.hp = a->H_operator ? HP_OPERATOR
         : (lowrank && !a->H_rowptr && !a->H_val) ? HP_LOWRANK
         : (dense && !a->H_rowptr) ? HP_DENSE : HP_CSR;
  P.lowrank_tail = lowrank && (P.hp == HP_DENSE || P.hp == HP_CSR);
  P.np1 = a->H_operator ? 1                      // [unused, p'Hp] written by the caller
          : lowrank ? ipx_lowrank_grid(a->LR_rows)
          : P.hp == HP_DENSE ? dense_grid(a->n) : (int)a->H_ntiles;
  P.xs_ncomp = (int)((a->H_ntiles + XS_SLICE - 1) / XS_SLICE);
  P.fused_hp = a->pb != nullptr && a->H_hmax > 0 && !a->H_operator;
  if (dense) {
    // dense Jacobian (`banded` = G^-1 in device memory, not a handle): the vector kernels
    // around the dense matvecs, whose workgroups leave the partials
    P.step1 = S1_VECTOR; P.proj = PJ_DENSE; P.step2 = S2_VECTOR;
    P.np2 = (int)a->vec_grid; P.np3 = dense_grid(a->n); P.np4 = dense_grid(a->m);
    return P;
  }
  const bool fused_ar = a->r_next != nullptr && a->A_own != nullptr && a->A_span > 0 && !a->lb &&
                        a->m > 0;
  // solver_kind 1 with the group tables present: the fused box-Schur projection
  const ipx_boxschur_args *b = a->solver_kind == 1 ? (const ipx_boxschur_args *)a->banded : nullptr;
  const bool box = b && a->m > 0 && !fused_ar && b->gcol != nullptr && b->grp != nullptr &&
                   b->up != nullptr;
  const bool tail = a->solver_kind == 0 && a->At_vown && a->At_qv > 0;
  P.step1 = fused_ar ? S1_FUSED_AR : box ? S1_BOX : S1_VECTOR;
  P.proj = a->m <= 0 ? PJ_NONE : box ? PJ_BOX : tail ? PJ_SOLVE_TAIL : PJ_SOLVE_SPMV;
  P.step2 = P.fused_hp ? S2_FUSED_HP : S2_VECTOR;
  P.no_xn2 = fused_ar && a->no_radius != 0;
  P.np4 = a->m > 0 ? ipx_banded_resid_count(a->solver_kind == 1 ? (b ? b->inner : nullptr)
                                                                : a->banded) : 1;
  // the projection half as one launch: asked for, every table bound, and no resident launch
  if (a->fused_proj != 0 && fused_ar && P.proj == PJ_SOLVE_TAIL && a->At_ell_row &&
      a->At_ell_val && a->A_ell_val && a->A_ell_off16 && a->A_rowfirst && a->P_win &&
      a->r_where && a->n % 2 == 0 && !ipx_cg_resident_ok(a) &&
      ipx_banded_fused_proj_ok(a->banded, (int)a->A_rl, a->P_nspan, (int)a->At_qv) == IPX_OK)
    P.proj = PJ_STEP1_SOLVE_TAIL;
  const int xs_wgs = P.proj == PJ_STEP1_SOLVE_TAIL ? P.np4 : (int)a->A_ntiles;   // who folds them
  P.xsums = a->xsums != nullptr && fused_ar && P.fused_hp && a->no_radius == 0 &&
            P.xs_ncomp <= xs_wgs && P.xs_ncomp <= XS_STRIDE;
  P.guard = P.xsums && a->radius_guard != 0 && a->rguard != nullptr && !ipx_cg_resident_ok(a);
  if (box) {
    const int64_t per = (int64_t)IPX_BLOCK * step1_box_rounds(b);
    P.np2 = (int)((b->ng + b->ngen + per - 1) / per);
    P.np3 = ipx_boxschur_project_count(b);
  } else {
    P.np2 = P.proj == PJ_STEP1_SOLVE_TAIL ? P.np4 : fused_ar ? (int)a->A_ntiles : (int)a->vec_grid;
    P.np3 = P.proj == PJ_SOLVE_TAIL || P.proj == PJ_STEP1_SOLVE_TAIL ? P.np4 : (int)a->At_ntiles;
  }
  return P;
}

// ---- kernel tables: every instantiation of the three templated loop kernels ----------------
// One function per kernel maps the runtime choices to a kernel (NULL: no such combination).  The
// PEER forms take the peer job where the others take an empty struct: two pointer types each.

// k_cg_step1_box<PEER, MODE>: the three group-table forms (csrc/boxschur.hip) x PEER -- 6.
template <bool PEER> using Step1BoxFn = decltype(&k_cg_step1_box<PEER, IPX_GROUPS_FULL>);
template <bool PEER> Step1BoxFn<PEER> step1_box_kernel(int group_mode) {
  switch (group_mode) {
    case IPX_GROUPS_AFFINE: return k_cg_step1_box<PEER, IPX_GROUPS_AFFINE>;
    case IPX_GROUPS_UNIT: return k_cg_step1_box<PEER, IPX_GROUPS_UNIT>;
    default: return k_cg_step1_box<PEER, IPX_GROUPS_FULL>;
  }
}

// k_cg_step1_ar<QS, FT_NNZ, XN, C16, PEER>: 8 forms x QS = 2, 4, 6, 8 (the column span of a row
// tile in blocks of IPX_BLOCK, rounded up to even; a wider span has no kernel) -- 32.
//   XN   0: ||x + alpha p||^2 from x and p;  1: not formed (LoopPlan.no_xn2);  2: from the
//        carried sums, x and p not read;  3: the radius guard (LoopPlan.guard), 1 + the bound T
//   C16  16-bit column offsets (ipx_cg_args.A_col16)
//   one GPU   XN 0, 1, 2, 3  x  C16 0, 1
//   PEER      XN 0, 1 with C16 only: peer_fusable admits no pattern without the 16-bit tables,
//             and the carried sums are one GPU's (the ranks' test needs the all-reduced sum)
template <bool PEER> using Step1ArFn = decltype(&k_cg_step1_ar<2, FT_NNZ, 0, true, PEER>);
template <bool PEER, int QS> Step1ArFn<PEER> step1_ar_forms(int xn, bool c16) {
  if constexpr (PEER) {
    static constexpr Step1ArFn<true> K[4] = {k_cg_step1_ar<QS, FT_NNZ, 0, true, true>,
                                  k_cg_step1_ar<QS, FT_NNZ, 1, true, true>, nullptr, nullptr};
    return c16 ? K[xn] : nullptr;
  } else {
    static constexpr Step1ArFn<false> K[4][2] = {
        {k_cg_step1_ar<QS, FT_NNZ, 0, false, false>, k_cg_step1_ar<QS, FT_NNZ, 0, true, false>},
        {k_cg_step1_ar<QS, FT_NNZ, 1, false, false>, k_cg_step1_ar<QS, FT_NNZ, 1, true, false>},
        {k_cg_step1_ar<QS, FT_NNZ, 2, false, false>, k_cg_step1_ar<QS, FT_NNZ, 2, true, false>},
        {k_cg_step1_ar<QS, FT_NNZ, 3, false, false>, k_cg_step1_ar<QS, FT_NNZ, 3, true, false>}};
    return K[xn][c16 ? 1 : 0];
  }
}
template <bool PEER> Step1ArFn<PEER> step1_ar_kernel(int qs, int xn, bool c16) {
  switch ((qs + 1) / 2) {
    case 1: return step1_ar_forms<PEER, 2>(xn, c16);
    case 2: return step1_ar_forms<PEER, 4>(xn, c16);
    case 3: return step1_ar_forms<PEER, 6>(xn, c16);
    case 4: return step1_ar_forms<PEER, 8>(xn, c16);
  }
  return nullptr;
}

// k_cg_step2_hp<HAS_DIAG, Q, QS, BOX, C16, PEER, XSUM, GUARD>: 10 forms x HAS_DIAG x (Q, QS) -- 40.
//   (Q, QS)  (3, 3) for short row tiles -- 3 nonzeros per row -> 683 rows: 3 elements per lane,
//            fewer registers -- else (4, 5)
//   one GPU  BOX 0, 1  x  C16 0, 1 without XSUM;  XSUM x C16 0, 1 without BOX: the carried sums
//            need the fused step1, which a box excludes (a box wins: XSUM is not looked at);
//            GUARD x C16 0, 1 without BOX and XSUM (the radius guard, where XSUM would apply)
//   PEER     BOX 0, 1 with C16 only (peer_fusable), never XSUM (the carried sums are one GPU's)
//   The four GUARD x C16 instantiations form the column offsets of flagged tiles
//   (ROWLEN_SHIFTED); no instantiation was added for that.
template <bool PEER> using Step2HpFn = decltype(&k_cg_step2_hp<true, 4, 5, false, true, PEER>);
template <bool PEER, bool D, int Q, int QS>
Step2HpFn<PEER> step2_hp_forms(bool box, bool c16, bool xsum, bool guard) {
  if constexpr (PEER) {
    if (!c16) return nullptr;
    return box ? k_cg_step2_hp<D, Q, QS, true, true, true>
               : k_cg_step2_hp<D, Q, QS, false, true, true>;
  } else {
    static constexpr Step2HpFn<false> K[4][2] = {
        {k_cg_step2_hp<D, Q, QS, false, false, false>, k_cg_step2_hp<D, Q, QS, false, true, false>},
        {k_cg_step2_hp<D, Q, QS, true, false, false>, k_cg_step2_hp<D, Q, QS, true, true, false>},
        {k_cg_step2_hp<D, Q, QS, false, false, false, true>,
         k_cg_step2_hp<D, Q, QS, false, true, false, true>},
        {k_cg_step2_hp<D, Q, QS, false, false, false, false, true>,
         k_cg_step2_hp<D, Q, QS, false, true, false, false, true>}};
    return K[box ? 1 : guard ? 3 : xsum ? 2 : 0][c16 ? 1 : 0];
  }
}
template <bool PEER>
Step2HpFn<PEER> step2_hp_kernel(bool diag, bool small, bool box, bool c16, bool xsum,
                                bool guard) {
  if (diag)
    return small ? step2_hp_forms<PEER, true, 3, 3>(box, c16, xsum, guard)
                 : step2_hp_forms<PEER, true, 4, 5>(box, c16, xsum, guard);
  return small ? step2_hp_forms<PEER, false, 3, 3>(box, c16, xsum, guard)
               : step2_hp_forms<PEER, false, 4, 5>(box, c16, xsum, guard);
}

// ---- single launches --------------------------------------------------------------------

// np2: the plan's (blocks of the kernel)
template <bool PEER>
int launch_step1_box(const ipx_cg_args *a, int it, const double *p1, int np1, int np2,
                     const OwnRanges &own, typename peer_arg<PEER>::type pj, hipStream_t st) {
  const ipx_boxschur_args *b = (const ipx_boxschur_args *)a->banded;
  const ipx_group_tab T = ipx_boxschur_tab(b);
  hipLaunchKernelGGL(step1_box_kernel<PEER>(ipx_group_mode(T)), dim3(ipx_xcd_grid(np2)),
                     dim3(IPX_BLOCK), 0, st, a->state, it & 1, p1, np1, a->x, a->p, a->r, a->Hp,
                     a->lb, a->ub, a->part2, np2, (int)b->ng, (int)b->ngen, T, b->gen_cols,
                     (int)b->ny, b->up, own, step1_box_rounds(b), pj);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

// step1 + A.r in one launch (see k_cg_step1_ar): r_next <- r + alpha Hp, w <- A r_next.
// no_xn2: x and p are not read, 16 of the kernel's 56 MB at n = 1e6.  carried (a finite radius,
// no box): the lean form that folds the carried sums' raw partials instead (XN = 2).  guard: the
// radius guard's form (XN = 3), which takes the guard's words where XN = 2 takes the folded sums.
template <bool PEER>
int launch_step1_ar(const ipx_cg_args *a, const LoopPlan &P, int it, const double *p1, int np1,
                    bool no_xn2, bool carried, bool guard, typename peer_arg<PEER>::type pj,
                    hipStream_t st) {
  if (carried && (PEER || no_xn2 || !a->xsums)) return IPX_EINVAL;
  if (guard && (PEER || no_xn2 || carried || !a->rguard)) return IPX_EINVAL;
  if (a->A_tile_nnz != 0) return IPX_EINVAL;    // (the 1024-nonzero tile form was removed)
  const int qs = (int)((a->A_span + IPX_BLOCK - 1) / IPX_BLOCK);
  const auto k = step1_ar_kernel<PEER>(qs, guard ? 3 : carried ? 2 : no_xn2 ? 1 : 0,
                                       a->A_col16 != nullptr);
  if (!k) return IPX_EINVAL;      // (a wider span; PEER without the 16-bit tables: peer_fusable)
  const int nraw = carried ? (int)a->H_ntiles : 0;
  hipLaunchKernelGGL(k, dim3(ipx_xcd_grid((int)a->A_ntiles)), dim3(IPX_BLOCK), 0, st, (int)a->n,
                     a->state, it & 1, p1, np1, a->x, a->p, a->r, a->r_next, a->Hp, a->A_rowptr,
                     a->A_colidx, a->A_val, a->A_tiles, (int)a->A_ntiles, a->A_own, a->w,
                     a->part2, (const uint16_t *)a->A_col16, pj, carried ? a->xsums : nullptr,
                     nraw, guard ? a->rguard : carried ? a->xsums + 3 * nraw + 1 : nullptr,
                     carried ? P.xs_ncomp : 0, it);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

// step2 + H.p in one launch (see k_cg_step2_hp); iteration `it` reads the halo copies of
// parity it & 1 and leaves those of p_next in the other one.  xs.raw == NULL: the kernel
// without the carried sums.
template <bool PEER>
int launch_step2_hp(const ipx_cg_args *a, int it, int mode, const double *p2, int np2,
                    const double *p3, int np3, const double *p4, int np4,
                    typename peer_arg<PEER>::type pj, const ipx_xsums_job &xs, hipStream_t st,
                    const double *g = nullptr) {
  const bool guard = (mode & 8) != 0;           // (the radius guard: xs.in = its three words)
  const bool xsum = !guard && xs.raw != nullptr && (xs.write != 0 || (mode & 4) != 0);
  if ((mode & 4) && (!xsum || !xs.in || PEER || a->lb)) return IPX_EINVAL;
  if (guard && (!xs.raw || !xs.in || xs.write || (mode & 4) || PEER || a->lb)) return IPX_EINVAL;
  // H_tile_rows: the longest tile's row count (set by the host binding)
  const bool small = a->H_tile_rows > 0 && a->H_tile_rows + 2 * a->H_hmax <= 3 * IPX_BLOCK;
  const bool c16 = a->H_col16 != nullptr && a->H_rowlen != nullptr;
  const auto k = step2_hp_kernel<PEER>(a->H_diag != nullptr, small, a->lb != nullptr, c16, xsum,
                                       guard);
  if (!k) return IPX_EINVAL;      // (PEER without the 16-bit tables: see peer_fusable)
  const int64_t half = a->H_ntiles * 2 * a->H_hmax;
  const double *pb_in = a->pb + (it & 1) * half;
  double *pb_out = a->pb + ((it + 1) & 1) * half;
  double *g_halo = PEER ? a->r : nullptr;
  hipLaunchKernelGGL(k, dim3(ipx_xcd_grid((int)a->H_ntiles)), dim3(IPX_BLOCK), 0, st, (int)a->n,
                     a->state, it & 1, mode, p2, np2, p3, np3, p4, np4, a->x, a->p,
                     g ? g : (const double *)a->r, a->H_rowptr, a->H_colidx, a->H_val, a->H_tiles,
                     (int)a->H_ntiles, a->H_diag, a->Hp, a->part1, (int)a->H_hmax, pb_in, pb_out,
                     (const uint16_t *)a->H_col16, a->H_rowlen, pj, g_halo, xs);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

// the tag of the carried sums (ipx_cg_args.xsums), NULL without them
double *xsums_tag(const ipx_cg_args *a) {
  return a->xsums ? a->xsums + 3 * a->H_ntiles : nullptr;
}

// p at the row-tile boundaries of H (the fused step2 + H.p kernel reads its neighbours' OLD p
// there) from the current a->p
int launch_save_pb(const ipx_cg_args *a, hipStream_t st) {
  const int tot = (int)(a->H_ntiles * 2 * a->H_hmax);
  hipLaunchKernelGGL(k_cg_save_pb, dim3((tot + IPX_BLOCK - 1) / IPX_BLOCK), dim3(IPX_BLOCK), 0, st,
                     a->p, a->H_tiles, (int)a->H_ntiles, (int)a->H_hmax, a->pb, xsums_tag(a));
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

// the low-rank term behind an H.p that left Hp (has_base) or none (H is that term + diagonal)
int launch_lowrank(const ipx_cg_args *a, bool has_base, const double *guard, hipStream_t st) {
  return ipx_lowrank_cg_launch(a->n, a->LR_rows, (int)a->LR_mem, a->LR_W, a->LR_state, a->LR_part,
                               a->p, a->Hp, a->H_diag, has_base ? 1 : 0, a->part1, guard, st);
}

// Unfused H.p in the plan's form; when the fused step2 + H.p kernel is enabled it also saves the
// tile boundaries of the p it was given (that kernel's halo source).
int launch_hp(const ipx_cg_args *a, const LoopPlan &P, const double *guard, hipStream_t st) {
  int rc = IPX_OK;
  switch (P.hp) {
    case HP_OPERATOR:
      return IPX_OK;
    case HP_LOWRANK:
      return launch_lowrank(a, false, guard, st);
    case HP_DENSE: {
      int np = 0;
      rc = ipx_dense_gemv_launch((int)a->n, (int)a->n, a->H_val, a->n, a->p, 1.0, a->H_diag, 0.0,
                                 nullptr, a->Hp, a->part1, &np, guard, st);
      break;
    }
    case HP_CSR: {
      ipx_csr_view H{(int)a->n, (int)a->n, a->H_rowptr, a->H_colidx, a->H_val, a->H_tiles,
                     (int)a->H_ntiles};
      rc = ipx_spmv_launch(H, a->p, 1.0, a->H_diag, 0.0, nullptr, a->Hp, a->part1, guard, st);
      break;
    }
  }
  if (!rc && P.lowrank_tail) rc = launch_lowrank(a, true, guard, st);
  if (rc || P.hp != HP_CSR || !P.fused_hp) return rc;
  return launch_save_pb(a, st);
}

// Host side of k_compact_partials: queue arrays, launch once, hand back the
// (pointer, entries per half) the consumer should fold.
struct Compactor {
  const ipx_cg_args *a;
  CompactJob job;
  const double *guard;          // the stop word, or NULL: compact whatever it says
  int n = 0, used = 0;
  Compactor(const ipx_cg_args *args, const double *g) : a(args), guard(g) { job.first[0] = 0; }
  // returns true (and rewrites ptr / count) when the array will be compacted
  bool add(const double *&ptr, int &count, int halves, int limit) {
    if (!a->fold_ws || count <= limit || n >= 3) return false;
    const int G = (count + 1023) / 1024;
    if (used + halves * G > IPX_FOLD_WS_DOUBLES) return false;
    job.in[n] = ptr; job.count[n] = count; job.halves[n] = halves; job.G[n] = G;
    job.out[n] = a->fold_ws + used;
    job.first[n + 1] = job.first[n] + halves * G;
    ptr = a->fold_ws + used;
    count = G;
    used += halves * G;
    ++n;
    return true;
  }
  int launch(hipStream_t st) {
    if (n == 0) return IPX_OK;
    for (int k = n; k < 3; ++k) job.first[k + 1] = job.first[n];
    hipLaunchKernelGGL(k_compact_partials, dim3(job.first[n]), dim3(IPX_BLOCK), 0, st, job, guard);
    IPX_CHECK_LAUNCH();
    n = 0;                       // `used` keeps growing: later arrays get fresh scratch
    job.first[0] = 0;
    return IPX_OK;
  }
};

// ---- the two halves of an iteration -------------------------------------------------------

// What differs between the drivers, besides where the partials a half folds come from (its
// arguments: an array with its count, one all-reduced entry, a rank's own window of an array).
struct HalfArgs {
  int it;
  // step2's mode bits: 1 no ||x + alpha p||^2 (LoopPlan.no_xn2), 2 no orthogonality test, 4 the
  // radius test from the carried sums, 8 from the radius guard's bound (no sums; xs.in = rguard).
  // The projection half reads 1, 4 and 8 (for its step1)
  int mode;
  const double *guard;                  // the stop word, for the launches that take one
  const OwnRanges *own = nullptr;       // the rank's own entries (sharded loop); NULL: every entry
  const ipx_peer_job *peer = nullptr;   // collectives in the kernels' prologues (sharded, fuse_comm)
  Compactor *cmp = nullptr;             // arrays too long to fold directly are compacted first
  // the carried sums the fused step2 + H.p writes and reads (the batch loop's alone)
  ipx_xsums_job xs{nullptr, nullptr, it, 0};
  hipEvent_t *ev = nullptr;             // ipx_cg_iterate_timed's events of this iteration
  // PJ_STEP1_SOLVE_TAIL: the roles of r and r_next alternate inside a batch -- flip = the
  // current r lives in r_next (and g goes to r); first = the batch's first iteration
  bool flip = false, first = true;
  const double *g = nullptr;            // where this iteration's g is (NULL: a->r)
};
#define MARK(i) do { if (h.ev) (void)hipEventRecord(h.ev[i], st); } while (0)

// step1 in its form (folding the np1 entries of p'Hp at p1 + np1), w = A r where step1 did not
// form it, the solve in its form, g = r - A'v where the solve did not form it.  Hands back how
// many partials per half it left in part2, part3 and part4.
int launch_projection_half(const ipx_cg_args *a, const LoopPlan &P, const HalfArgs &h,
                           const double *p1, int np1, int *np2, int *np3, int *np4,
                           hipStream_t st) {
  MARK(0);
  int rc;
  if (h.cmp) {
    h.cmp->add(p1, np1, 2, 2048);      // beyond what a consumer folds in one or two rounds
    rc = h.cmp->launch(st);
    if (rc) return rc;
  }
  if (P.proj == PJ_STEP1_SOLVE_TAIL) {
    if (h.peer || h.own) return IPX_EINVAL;
    const bool carried = (h.mode & 4) != 0, guarded = (h.mode & 8) != 0;
    if (carried && ((h.mode & 1) || !a->xsums)) return IPX_EINVAL;
    if (guarded && ((h.mode & 5) || !a->rguard)) return IPX_EINVAL;
    const int nraw = carried ? (int)a->H_ntiles : 0;
    ipx_fused_proj_job J{};
    J.st = a->state; J.parity = h.it & 1; J.p1 = p1 + np1; J.np1 = np1;
    J.r_in = h.flip ? a->r_next : a->r; J.Hp = a->Hp; J.g_out = h.flip ? a->r : a->r_next;
    J.xn = guarded ? 3 : carried ? 2 : (h.mode & 1) ? 1 : 0;
    J.x = a->x; J.p = a->p; J.part2 = a->part2;
    J.xs_raw = carried ? a->xsums : nullptr; J.nraw = nraw;
    J.xs_comp = guarded ? a->rguard : carried ? a->xsums + 3 * nraw + 1 : nullptr;
    J.ncomp = carried ? P.xs_ncomp : 0; J.it = h.it;
    J.A_ell_val = a->A_ell_val; J.A_ell_off16 = (const uint16_t *)a->A_ell_off16;
    J.contig = a->A_contig != 0;
    J.A_rowfirst = a->A_rowfirst; J.rl = (int)a->A_rl; J.win = a->P_win; J.n = a->n;
    J.vown = a->At_vown; J.qv = (int)a->At_qv; J.ell_row = a->At_ell_row; J.ell_val = a->At_ell_val;
    J.v = a->v; J.part3 = a->part3; J.part4 = a->part4;
    J.where = a->r_where; J.first = h.first ? 1 : 0; J.dest = h.flip ? 0 : 1;
    MARK(1); MARK(2);
    int np = 0;
    rc = ipx_banded_fused_proj_launch(a->banded, J, &np, st);
    if (rc) return rc;
    *np2 = *np3 = *np4 = np;
    MARK(3); MARK(4); MARK(5);
    return IPX_OK;
  }
  const bool fuse1 = P.step1 == S1_FUSED_AR;
  const OwnRanges own = h.own ? *h.own : own_all(a->n);
  switch (P.step1) {
    case S1_FUSED_AR:
      MARK(1);
      rc = h.peer ? launch_step1_ar<true>(a, P, h.it, p1, np1, h.mode & 1, h.mode & 4, h.mode & 8,
                                          *h.peer, st)
                  : launch_step1_ar<false>(a, P, h.it, p1, np1, h.mode & 1, h.mode & 4, h.mode & 8,
                                           ipx_no_peer{}, st);
      if (rc) return rc;
      MARK(2);
      break;
    case S1_BOX:
      rc = h.peer ? launch_step1_box<true>(a, h.it, p1, np1, P.np2, own, *h.peer, st)
                  : launch_step1_box<false>(a, h.it, p1, np1, P.np2, own, ipx_no_peer{}, st);
      if (rc) return rc;
      MARK(1);
      break;
    case S1_VECTOR:
      if (h.peer) return IPX_EINVAL;                 // (no PEER form: see peer_fusable)
      hipLaunchKernelGGL(k_cg_step1, dim3(ipx_xcd_grid((int)a->vec_grid)), dim3(VB), 0, st, a->n,
                         a->state, h.it & 1, p1, np1, a->x, a->p, a->r, a->Hp, a->lb, a->ub,
                         a->part2, (int)a->vec_grid, own);
      IPX_CHECK_LAUNCH();
      MARK(1);
      break;
  }
  *np2 = P.np2;
  *np3 = P.np3;
  *np4 = P.np4;
  const double *r_in = fuse1 ? a->r_next : a->r;      // what g = r - A'v reads
  switch (P.proj) {
    case PJ_NONE:
      break;
    case PJ_BOX: {
      // simple (box) rows eliminated analytically and never multiplied as matrix rows:
      // g = r - A'(A A')^-1 A r in one call (csrc/boxschur.hip); a rank's kernels count its own
      // entries only (element mask), so its own sums are the sums over ALL their partials
      int32_t n3 = 0, n4 = 0;
      rc = ipx_boxschur_project_from((const ipx_boxschur_args *)a->banded, a->r, a->r, a->part3,
                                     &n3, a->part4, &n4, h.guard, 1, st, h.own);
      if (rc) return rc;
      *np3 = n3;
      *np4 = n4;
      MARK(2); MARK(3); MARK(4); MARK(5);
      break;
    }
    case PJ_SOLVE_TAIL:
    case PJ_SOLVE_SPMV: {
      if (!fuse1) {
        ipx_csr_view A{(int)a->m, (int)a->n, a->A_rowptr, a->A_colidx, a->A_val, a->A_tiles,
                       (int)a->A_ntiles};
        rc = ipx_spmv_launch(A, a->r, 1.0, nullptr, 0.0, nullptr, a->w, nullptr, h.guard, st);
        if (rc) return rc;
        MARK(2);
      }
      // v = (AA')^-1 w, and ||A g||^2 for the orthogonality test as the constraint-space
      // residual ||w - (A A') v||^2 from the same launch (see k_correct_oop / k_band_residual)
      if (P.proj == PJ_SOLVE_TAIL) {
        // decoupled banded solve with g = r - A'v as its tail (one launch for both);
        // ||g||^2 partials are then per workgroup of that kernel
        rc = ipx_banded_solve_resid_atv_launch(a->banded, a->w, a->v, a->part4, np4, a->At_rowptr,
                                               a->At_colidx, a->At_val, r_in, a->r, a->At_vown,
                                               (int)a->At_qv, a->part3, h.guard, st,
                                               a->At_ell_row, a->At_ell_val, a->n);
        if (rc) return rc;
        *np3 = *np4;
        MARK(3);
        MARK(4);
      } else {
        if (a->solver_kind == 1)    // box rows eliminated analytically, banded Schur complement
          rc = ipx_boxschur_solve((const ipx_boxschur_args *)a->banded, a->w, a->v, a->part4, np4,
                                  h.guard, st);
        else
          rc = ipx_banded_solve_resid_launch(a->banded, a->w, a->v, a->part4, np4, h.guard, st);
        if (rc) return rc;
        MARK(3);
        // r = r - A'v  (g_next), partials of ||g||^2
        ipx_csr_view At{(int)a->n, (int)a->m, a->At_rowptr, a->At_colidx, a->At_val, a->At_tiles,
                        (int)a->At_ntiles};
        rc = ipx_spmv_launch(At, a->v, -1.0, nullptr, 1.0, r_in, a->r, a->part3, h.guard, st);
        if (rc) return rc;
        MARK(4);
      }
      MARK(5);
      break;
    }
    case PJ_STEP1_SOLVE_TAIL:
      return IPX_EINVAL;                             // (launched above)
    case PJ_DENSE: {
      // Dense Jacobian (BASELINE config 2): A (m x n) and A' (n x m) row major in A_val /
      // At_val, `banded` = G^-1 (M x M, M = m rounded up to 32; w and v are M long with a zero
      // tail).  Four matvecs, whose epilogues carry the reductions: w = A r, v = G^-1 w,
      // g = r - A'v, t = A g (the reference's orthogonality measure, projections.py:52, literally)
      const int n = (int)a->n, m = (int)a->m, M = ((m + 31) / 32) * 32;
      int np = 0;
      rc = ipx_dense_gemv_launch(m, n, a->A_val, n, a->r, 1.0, nullptr, 0.0, nullptr, a->w,
                                 nullptr, &np, h.guard, st);
      if (rc) return rc;
      rc = ipx_dense_gemv_launch(M, M, (const double *)a->banded, M, a->w, 1.0, nullptr, 0.0,
                                 nullptr, a->v, nullptr, &np, h.guard, st);
      if (rc) return rc;
      rc = ipx_dense_gemv_launch(n, m, a->At_val, m, a->v, -1.0, nullptr, 1.0, a->r, a->r,
                                 a->part3, np3, h.guard, st);              // g = r - A'v, ||g||^2
      if (rc) return rc;
      rc = ipx_dense_gemv_launch(m, n, a->A_val, n, a->r, 1.0, nullptr, 0.0, nullptr, a->t,
                                 a->part4, np4, h.guard, st);              // ||A g||^2
      if (rc) return rc;
      break;
    }
  }
  return IPX_OK;
}

// Compaction of the long partial arrays, step2 in its form (folding ||x + alpha p||^2 and the
// violations at p2, ||g||^2 at p3, ||A g||^2 at p4), H.p where step2 did not form it, the
// low-rank tail, and the tile boundaries of p where the fused kernel will want them.
int launch_update_half(const ipx_cg_args *a, const LoopPlan &P, const HalfArgs &h,
                       const double *p2, int np2, const double *p3, int np3, const double *p4,
                       int np4, hipStream_t st) {
  int rc;
  if (h.cmp) {
    // every workgroup folds all of them: at n = 1.6e7 the 6000 uncompacted ||g||^2 partials
    // doubled what a workgroup of the fused kernel reads (495 us on its own, 226 us in the loop)
    // (bit 4: the folded sums in its place; bit 8: the guard's bound, nothing folded)
    if (!(h.mode & 13)) h.cmp->add(p2, np2, 2, 1024);
    h.cmp->add(p3, np3, 2, 2048);
    if (!(h.mode & 2)) h.cmp->add(p4, np4, 1, 1024);
    rc = h.cmp->launch(st);
    if (rc) return rc;
  }
  // g: a->r, or under PJ_STEP1_SOLVE_TAIL whichever of r / r_next this iteration's launch wrote
  const double *g = h.g ? h.g : a->r;
  if (P.step2 == S2_FUSED_HP) {
    MARK(6);
    rc = h.peer ? launch_step2_hp<true>(a, h.it, h.mode, p2, np2, p3, np3, p4, np4, *h.peer, h.xs,
                                        st)
                : launch_step2_hp<false>(a, h.it, h.mode, p2, np2, p3, np3, p4, np4,
                                         ipx_no_peer{}, h.xs, st, g);
    if (!rc && P.lowrank_tail) rc = launch_lowrank(a, true, h.guard, st);
  } else {
    if (h.peer) return IPX_EINVAL;                   // (no PEER form: see peer_fusable)
    hipLaunchKernelGGL(k_cg_step2, dim3(ipx_xcd_grid((int)a->vec_grid)), dim3(VB), 0, st, a->n,
                       a->state, h.it & 1, h.mode, p2, np2, p3, np3, p4, np4, a->x, a->p, g,
                       (int)a->vec_grid);
    IPX_CHECK_LAUNCH();
    MARK(6);
    rc = launch_hp(a, P, h.guard, st);
  }
  if (rc) return rc;
  MARK(7);
  return IPX_OK;
}
#undef MARK

// Enqueue iterations it_begin .. it_end-1.  Never synchronises.  ev (ipx_cg_iterate_timed): eight
// events per iteration, recorded around its kernel classes.
int cg_iterate(const ipx_cg_args *a, const LoopPlan &P, int32_t it_begin, int32_t it_end,
               hipStream_t st, hipEvent_t *ev) {
  if (P.proj == PJ_DENSE) {
    if (ev) return IPX_EINVAL;
  } else if (!ev && it_end > it_begin && ipx_cg_resident_ok(a)) {
    // small banded problems (one CU per workgroup of the solve): the whole batch as ONE
    // resident launch (csrc/resident.hip), which leaves x, p, r, Hp, the state block and the
    // partial arrays as these launches would -- the tile boundaries of p for the fused step2 +
    // H.p kernel (an event handler's resume, a later batch on the separate launches) follow it
    int rc = ipx_cg_resident_launch(a, it_begin, it_end, P.np1, P.np2, P.np3, P.np4, st);
    if (rc || !P.fused_hp) return rc;
    return launch_save_pb(a, st);
  }
  const double *guard = a->state + ST_STOP;
  // a batch whose fused step2 + H.p launches run without the carried sums (trust radius +inf)
  // changes x and p and leaves none: their tag is void from here on (one launch per batch)
  if (a->xsums && !P.xsums && it_end > it_begin) {
    hipLaunchKernelGGL(k_xsums_void, dim3(1), dim3(1), 0, st, xsums_tag(a));
    IPX_CHECK_LAUNCH();
  }
  for (int it = it_begin; it < it_end; ++it) {
    // a finite radius: the test is formed from the sums the previous iteration's fused step2 +
    // H.p kernel left (ipx_cg_args.xsums) -- inside a batch, or where the caller vouches for
    // the batch before; the fused step1 then reads neither x nor p.  The first iteration of a
    // call reads them as before.
    // Under the radius guard neither form runs: the test is decided from the bound T the
    // projection half leaves (mode bit 8), no sums are written and their tag is cleared.
    const bool carried = P.xsums && !P.guard && (it > it_begin || a->xsums_carry != 0);
    Compactor cmp(a, guard);
    HalfArgs h{it, (P.proj == PJ_NONE ? 2 : 0) | (P.no_xn2 ? 1 : 0) | (carried ? 4 : 0) |
                       (P.guard ? 8 : 0), guard};
    if (P.proj != PJ_DENSE) h.cmp = &cmp;            // (the dense loop never compacted)
    // the fused step2 + H.p writes the sums (or voids their tag) and, carried, reads the sums
    // the fused step1 folded (in part2's place)
    h.xs = ipx_xsums_job{a->xsums,
                         P.guard ? a->rguard : carried ? a->xsums + 3 * a->H_ntiles + 1 : nullptr,
                         it, P.xsums && !P.guard ? 1 : 0};
    h.ev = ev;
    h.first = it == it_begin;
    h.flip = P.proj == PJ_STEP1_SOLVE_TAIL && ((it - it_begin) & 1) != 0;
    if (P.proj == PJ_STEP1_SOLVE_TAIL) h.g = h.flip ? a->r : a->r_next;
    int np2 = 0, np3 = 0, np4 = 0;
    int rc = launch_projection_half(a, P, h, a->part1, P.np1, &np2, &np3, &np4, st);
    if (rc) return rc;
    rc = launch_update_half(a, P, h, a->part2, np2, a->part3, np3, a->part4, np4, st);
    if (rc) return rc;
  }
  if (P.proj == PJ_STEP1_SOLVE_TAIL && it_end > it_begin) {
    // the current r back into a->r where the batch left it in r_next (an odd number of
    // projections ran: the word says so, whatever stopped the batch and where)
    hipLaunchKernelGGL(k_cg_settle_r, dim3(ipx_grid_for(a->n, VB * 4, 1024)), dim3(VB), 0, st, a->n,
                       a->r_where, (const double *)a->r_next, a->r);
    IPX_CHECK_LAUNCH();
  }
  return IPX_OK;
}
}  // namespace

IPX_STAMP_EXPORT(ipx_debug_stamps_cg, ipx_dbg_cg)

extern "C" {

int ipx_cg_state_size(void) { return ST_SIZE; }
// 2 workgroups per CU: measured best for step2 at n = 1e6 (9.3 us vs 10.8 us with 1024)
int ipx_cg_vec_grid(int64_t n) { return ipx_grid_for(n, VB * 2, 512); }

// Single kernels of the loop with explicit partial buffers, for drivers that
// interleave their own steps.
int ipx_cg_step1(int64_t n, double *state, int32_t it, const double *p1, int32_t np1,
                 const double *x, const double *p, double *r, const double *Hp, const double *lb,
                 const double *ub, double *part2, int32_t grid, void *stream) {
  if (n < 0 || !state || !p1 || !part2 || grid < 1) return IPX_EINVAL;
  hipLaunchKernelGGL(k_cg_step1, dim3(ipx_xcd_grid(grid)), dim3(VB), 0, (hipStream_t)stream, n,
                     state, it & 1, p1, np1, x, p, r, Hp, lb, ub, part2, grid, own_all(n));
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

int ipx_cg_step2(int64_t n, double *state, int32_t it, int32_t mode, const double *p2,
                 int32_t np2, const double *p3, int32_t np3, const double *p4, int32_t np4,
                 double *x, double *p, const double *g, int32_t grid, void *stream) {
  if (n < 0 || !state || grid < 1) return IPX_EINVAL;
  hipLaunchKernelGGL(k_cg_step2, dim3(ipx_xcd_grid(grid)), dim3(VB), 0, (hipStream_t)stream, n,
                     state, it & 1, mode, p2, np2, p3, np3, p4, np4, x, p, g, grid);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

static OwnRanges own_of(const ipx_shard2_ext *e) {
  OwnRanges o;
  for (int k = 0; k < 4; ++k) {
    o.lo[k] = k < e->nseg ? e->own_lo[k] : 0;
    o.hi[k] = k < e->nseg ? e->own_hi[k] : 0;
  }
  return o;
}

// The rank's own sums to `out`; with a peer mailbox (e->peer) all-reduced over the ranks in
// the same launch, and -- with_halo -- the halo of g (a->r) exchanged with the neighbours.
static int launch_pack(const ipx_cg_args *a, const ipx_shard2_ext *e, const RangeJob &job,
                       double *out, bool with_halo, hipStream_t st) {
  ipx_peer *peer = (ipx_peer *)e->peer;
  if (!peer) {
    hipLaunchKernelGGL(k_cg_range_pack, dim3(1), dim3(256), 0, st, job, out,
                       (const double *)nullptr);
    IPX_CHECK_LAUNCH();
    return IPX_OK;
  }
  if (peer->view.world > IPX_MAX_PEERS || !ipx_peer_ready(peer)) return IPX_EINVAL;
  HaloPlan hp;
  hp.nseg = 0;
  int64_t moved = 0;
  if (with_halo && peer->view.world > 1) {
    hp.nseg = (int)e->nseg;
    int64_t inl = 0, inr = 0, outl = 0, outr = 0;
    for (int k = 0; k < hp.nseg; ++k) {
      hp.seg_lo[k] = (int)e->seg_lo[k]; hp.seg_hi[k] = (int)e->seg_hi[k];
      hp.own_lo[k] = (int)e->own_lo[k]; hp.own_hi[k] = (int)e->own_hi[k];
      hp.send_left[k] = (int)e->send_left[k]; hp.send_right[k] = (int)e->send_right[k];
      if (hp.seg_lo[k] > hp.own_lo[k] || hp.own_hi[k] > hp.seg_hi[k] || hp.send_left[k] < 0 ||
          hp.send_right[k] < 0 || hp.send_left[k] + hp.send_right[k] > 2 * (hp.own_hi[k] - hp.own_lo[k]))
        return IPX_EINVAL;
      inl += hp.own_lo[k] - hp.seg_lo[k]; inr += hp.seg_hi[k] - hp.own_hi[k];
      outl += hp.send_left[k]; outr += hp.send_right[k];
    }
    // (the neighbours' capacities equal this rank's: one group, one ipx_peer_create argument)
    if (inl > peer->view.cap || inr > peer->view.cap || outl > peer->view.cap || outr > peer->view.cap)
      return IPX_EINVAL;
    moved = inl + inr + outl + outr;
    if (++peer->hseq == 0) ++peer->hseq;
  }
  if (++peer->seq == 0) ++peer->seq;
  const int halo_wg = hp.nseg ? (int)std::min<int64_t>(16, std::max<int64_t>(1, (moved + 511) / 512)) : 0;
  hipLaunchKernelGGL(k_cg_pack_comm, dim3(1 + halo_wg), dim3(256), 0, st, job, out, peer->view,
                     peer->seq, hp, a->r, peer->hseq, a->state);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

// zeros over the entries of `part` outside the given ranges (the p'Hp partials of halo tiles
// after an unfused H.p: the PEER form of k_cg_step1_box folds the whole array)
__global__ void __launch_bounds__(IPX_BLOCK)
k_zero_outside(double *__restrict__ part, int n, OwnRanges keep) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && !keep.has(i)) part[i] = 0.0;
}

// own sum of the p'Hp partials (second half of part1) over the segments' own row tiles
static int pack_hp(const ipx_cg_args *a, const ipx_shard2_ext *e, const LoopPlan &P,
                   hipStream_t st) {
  const int np1 = P.np1;
  RangeJob job;
  job.npieces = (int)e->nseg;
  job.active = 2;
  for (int pc = 0; pc < 4; ++pc)
    for (int q = 0; q < 4; ++q) { job.ptr[pc][q] = a->part1; job.count[pc][q] = 0; }
  for (int pc = 0; pc < (int)e->nseg; ++pc) {
    if (e->p1_hi[pc] > np1) return IPX_EINVAL;
    job.ptr[pc][1] = a->part1 + np1 + e->p1_lo[pc];
    job.count[pc][1] = (int)(e->p1_hi[pc] - e->p1_lo[pc]);
  }
  // NOT guarded by the stop flag: once an iteration has raised it, the remaining iterations
  // of the batch are no-ops but their all-reduces still run; re-packing the (unchanged)
  // own sums keeps the reduced values those of the iteration that stopped
  int rc = launch_pack(a, e, job, e->s1, false, st);
  if (rc || !e->peer || !e->fuse_comm || P.proj != PJ_BOX) return rc;
  // the prologue form of k_cg_step1_box folds ALL of part1's second half: zero the entries
  // an unfused H.p left for the tiles of halo rows
  OwnRanges keep;
  for (int k = 0; k < 4; ++k) {
    keep.lo[k] = k < (int)e->nseg ? e->p1_lo[k] : 0;
    keep.hi[k] = k < (int)e->nseg ? e->p1_hi[k] : 0;
  }
  hipLaunchKernelGGL(k_zero_outside, dim3((np1 + IPX_BLOCK - 1) / IPX_BLOCK), dim3(IPX_BLOCK), 0, st,
                     a->part1 + np1, np1, keep);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

// The collectives INSIDE the loop's own kernels (k_cg_step1_ar / k_cg_step2_hp, PEER forms): 3
// launches per iteration instead of 5.  Both need the fused step2 + H.p kernel in its 16-bit
// index form.
static bool peer_fusable(const ipx_cg_args *a, const ipx_shard2_ext *e, const LoopPlan &P) {
  ipx_peer *peer = (ipx_peer *)e->peer;
  if (!(peer && e->fuse_comm && peer->view.world > 1 && peer->view.world <= IPX_MAX_PEERS &&
        ipx_peer_ready(peer) && P.fused_hp && a->H_col16 && a->H_rowlen && a->m > 0))
    return false;
  // x-space problems: one segment, the fused step1 + A.r kernel (hence no box) in its 16-bit
  // index form, g = r - A'v as the solve's tail
  if (e->nseg == 1 && P.step1 == S1_FUSED_AR && a->A_col16 && P.proj == PJ_SOLVE_TAIL)
    return true;
  // the barrier problem's z-space: the projection without the box rows as matrix rows
  return P.proj == PJ_BOX && a->lb != nullptr;
}

// the segments' extents and their places in the mailboxes' halo areas
static int peer_job_geometry(const ipx_shard2_ext *e, const ipx_peer *peer, ipx_peer_job *pj) {
  pj->nseg = (int)e->nseg;
  int inl = 0, inr = 0, outl = 0, outr = 0;
  for (int k = 0; k < pj->nseg; ++k) {
    pj->seg_lo[k] = (int)e->seg_lo[k]; pj->own_lo[k] = (int)e->own_lo[k];
    pj->own_hi[k] = (int)e->own_hi[k]; pj->seg_hi[k] = (int)e->seg_hi[k];
    pj->send_left[k] = (int)e->send_left[k]; pj->send_right[k] = (int)e->send_right[k];
    if (pj->seg_lo[k] > pj->own_lo[k] || pj->own_hi[k] > pj->seg_hi[k] || pj->send_left[k] < 0 ||
        pj->send_right[k] < 0)
      return IPX_EINVAL;
    pj->off_l[k] = inl; pj->off_r[k] = inr; pj->push_l[k] = outl; pj->push_r[k] = outr;
    inl += pj->own_lo[k] - pj->seg_lo[k]; inr += pj->seg_hi[k] - pj->own_hi[k];
    outl += pj->send_left[k]; outr += pj->send_right[k];
  }
  const int64_t cap = peer->view.cap;
  return (inl > cap || inr > cap || outl > cap || outr > cap) ? IPX_EINVAL : IPX_OK;
}

// One local segment of an iteration of the PARTITIONED row-sharded loop (ipsolver/sharded.py
// FusedShardedCG).  The argument block describes the rank's extended local problem (own
// rows / variables plus halo copies): the halves are those of the single-GPU loop; what is
// specific is (a) their reduction inputs are the all-reduced scalars (e->s1, e->pack, one
// entry each) instead of the predecessor's partial arrays, and (b) the partials they leave
// are summed over the rank's own tiles only.
//   phase 0 (after the all-reduce of s1): the projection half, then the own sums of
//           ||x+ap||^2, #violations, ||g||^2, ||A g||^2 -> e->pack[0..4)
//   phase 1 (after the all-reduce of pack and the halo exchange of g): the update half, then
//           the own sum of p'Hp -> e->s1[1]
// fuse_comm: the collectives in the prologues of the halves' own kernels (HalfArgs.peer) -- the
// all-reduce of p'Hp in step1's, that of the four sums and the halo exchange of g in step2's;
// their inputs are then the rank's own windows of the partial arrays, and no pack launch runs.
static int shard2_segment(const ipx_cg_args *a, const ipx_shard2_ext *e, const LoopPlan &P,
                          int32_t phase, int32_t it, int32_t mode, void *stream, bool fuse_comm) {
  if (!a || !e || phase < 0 || phase > 1 || !e->s1 || !e->pack || a->solver_kind > 1 ||
      e->nseg < 1 || e->nseg > 4 || a->LR_W)
    return IPX_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const double *guard = a->state + ST_STOP;
  const bool boxp = P.proj == PJ_BOX;
  const OwnRanges own = own_of(e);
  int np2 = 0, np3 = 0, np4 = 0;
  if (fuse_comm) {
    ipx_peer *peer = (ipx_peer *)e->peer;
    ipx_peer_job pj{};
    pj.pv = peer->view;
    if (phase == 0) {
      // (every argument check comes BEFORE the sequence numbers move: a rank that returns
      // IPX_EINVAL must not leave its counters out of step with the group's)
      if (!boxp && (e->p1_hi[0] > P.np1 || e->p1_hi[0] < e->p1_lo[0])) return IPX_EINVAL;
      if (++peer->seq == 0) ++peer->seq;
      pj.seq = peer->seq;
      ++peer->fused;
      HalfArgs h{it, 0, guard};
      h.own = &own;
      h.peer = &pj;
      // box-Schur: the kernels count own entries only, all of part1's second half.  Else the
      // kernel folds [p1 + np1, p1 + 2 np1): hand it the own range as that window
      const int cnt = boxp ? P.np1 : (int)(e->p1_hi[0] - e->p1_lo[0]);
      const double *p1 = boxp ? a->part1 : a->part1 + P.np1 + e->p1_lo[0] - cnt;
      return launch_projection_half(a, P, h, p1, cnt, &np2, &np3, &np4, st);
    }
    // the own sums of p'Hp stay in part1 for the next step1
    if (e->p4_hi > P.np4) return IPX_EINVAL;
    if (!boxp && (e->p2_hi > (int)a->A_ntiles || e->p3_hi[0] > P.np4)) return IPX_EINVAL;
    int rc = peer_job_geometry(e, peer, &pj);
    if (rc) return rc;
    if (++peer->seq == 0) ++peer->seq;
    if (++peer->hseq == 0) ++peer->hseq;
    pj.seq = peer->seq;
    pj.hseq = peer->hseq;
    pj.pack_out = e->pack;
    ++peer->fused;
    HalfArgs h{it, mode, guard};
    h.peer = &pj;
    // (box-Schur: the kernels counted own entries only, the own sums are the whole arrays)
    const int64_t lo2 = boxp ? 0 : e->p2_lo, hi2 = boxp ? P.np2 : e->p2_hi;
    const int64_t lo3 = boxp ? 0 : e->p3_lo[0], hi3 = boxp ? P.np3 : e->p3_hi[0];
    return launch_update_half(a, P, h, a->part2 + lo2, (int)(hi2 - lo2), a->part3 + lo3,
                              (int)(hi3 - lo3), a->part4 + e->p4_lo, (int)(e->p4_hi - e->p4_lo), st);
  }
  if (phase == 0) {
    HalfArgs h{it, 0, guard};
    h.own = &own;
    int rc = launch_projection_half(a, P, h, e->s1, 1, &np2, &np3, &np4, st);
    if (rc) return rc;
    if (e->p4_hi > np4 || (!boxp && e->p2_hi > np2)) return IPX_EINVAL;
    RangeJob job;
    job.npieces = (int)e->nseg;
    job.active = 15;
    for (int pc = 0; pc < 4; ++pc)
      for (int q = 0; q < 4; ++q) { job.ptr[pc][q] = a->part2; job.count[pc][q] = 0; }
    // ||x+ap||^2, #violations and ||A g||^2 are single ranges (piece 0); ||g||^2 one per segment
    // (box-Schur projection: the kernels counted own entries only, the whole arrays)
    const int64_t p2lo = boxp ? 0 : e->p2_lo, p2hi = boxp ? np2 : e->p2_hi;
    job.ptr[0][0] = a->part2 + p2lo;        job.count[0][0] = (int)(p2hi - p2lo);
    job.ptr[0][1] = a->part2 + np2 + p2lo;  job.count[0][1] = (int)(p2hi - p2lo);
    job.ptr[0][3] = a->part4 + e->p4_lo;    job.count[0][3] = (int)(e->p4_hi - e->p4_lo);
    if (boxp) {
      job.ptr[0][2] = a->part3;
      job.count[0][2] = np3;
    } else {
      for (int pc = 0; pc < (int)e->nseg; ++pc) {
        if (e->p3_hi[pc] > np3) return IPX_EINVAL;
        job.ptr[pc][2] = a->part3 + e->p3_lo[pc];
        job.count[pc][2] = (int)(e->p3_hi[pc] - e->p3_lo[pc]);
      }
    }
    return launch_pack(a, e, job, e->pack, true, st);       // unguarded: see pack_hp
  }
  const HalfArgs h{it, mode, guard};
  int rc = launch_update_half(a, P, h, e->pack, 1, e->pack + 2, 1, e->pack + 3, 1, st);
  if (rc) return rc;
  return pack_hp(a, e, P, st);
}

int ipx_cg_shard2_segment(const ipx_cg_args *a, const ipx_shard2_ext *e, int32_t phase,
                          int32_t it, int32_t mode, void *stream) {
  if (!a) return IPX_EINVAL;
  return shard2_segment(a, e, plan_of(a), phase, it, mode, stream, false);
}

// Iterations [it_begin, it_end) of the sharded loop in ONE call: needs the peer mailbox
// (e->peer), through which the pack kernels all-reduce the scalars and exchange the halo of g
// themselves -- no collective call, no host between the iterations.
int ipx_cg_shard2_iterate(const ipx_cg_args *a, const ipx_shard2_ext *e, int32_t it_begin,
                          int32_t it_end, void *stream) {
  if (!a || !e || !e->peer || it_end < it_begin || a->LR_W) return IPX_EINVAL;
  const LoopPlan P = plan_of(a);
  // e->fuse_comm is the GROUP's decision (ipx_cg_shard2_fusable on every rank, the minimum
  // taken over the ranks by the caller): the two forms order the collectives of an iteration
  // differently, so a rank may not pick one from its own slice of the matrices
  const bool fuse = e->fuse_comm != 0;
  if (fuse && !peer_fusable(a, e, P)) return IPX_EINVAL;
  for (int it = it_begin; it < it_end; ++it) {
    int rc = shard2_segment(a, e, P, 0, it, 0, stream, fuse);
    if (rc) return rc;
    rc = shard2_segment(a, e, P, 1, it, 0, stream, fuse);
    if (rc) return rc;
  }
  return IPX_OK;
}

// The batch as one resident launch per rank (csrc/resident.hip, PEER form).
int ipx_cg_shard2_resident(const ipx_cg_args *a, const ipx_shard2_ext *e, int32_t it_begin,
                           int32_t it_end, void *stream) {
  if (!a || !e || a->LR_W) return IPX_EINVAL;
  return ipx_cg_shard2_resident_launch(a, e, it_begin, it_end, plan_of(a).np1, (hipStream_t)stream);
}

// p at the row-tile boundaries of H from the current a->p, where the fused step2 + H.p kernel
// is enabled (launch_save_pb)
int ipx_cg_save_pb(const ipx_cg_args *a, void *stream) {
  if (!a) return IPX_EINVAL;
  if (!plan_of(a).fused_hp) return IPX_OK;
  return launch_save_pb(a, (hipStream_t)stream);
}

// 1 when THIS rank's argument block allows the collectives in the prologues of the loop's own
// kernels (3 launches per iteration; peer_fusable: the tables are functions of the rank's
// slice of A and H).  The ranks must agree before anyone sets e->fuse_comm: the caller
// reduces this value with MIN over the group (ipsolver/sharded.py FusedShardedCG).
int ipx_cg_shard2_fusable(const ipx_cg_args *a, const ipx_shard2_ext *e) {
  if (!a || !e || !e->peer || a->LR_W) return 0;
  ipx_shard2_ext asked = *e;
  asked.fuse_comm = 1;
  return peer_fusable(a, &asked, plan_of(a)) ? 1 : 0;
}

// The own-range sum of the p'Hp partials on its own (priming the sharded loop).
int ipx_cg_shard2_fold_hp(const ipx_cg_args *a, const ipx_shard2_ext *e, void *stream) {
  if (!a || !e || !e->s1 || e->nseg < 1 || e->nseg > 4 || a->LR_W) return IPX_EINVAL;
  return pack_hp(a, e, plan_of(a), (hipStream_t)stream);
}

// The state block of a new call written ON THE DEVICE from reductions its priming left in
// device memory, so that a projected_cg call needs no host read before its first batch
// (reference qp_subproblem.py:502-542 evaluates these scalars on the host: five blocking reads
// here, ~0.3 ms of a call's fixed cost).  red[idx[.]]:
//   0: ||x0||^2;   1, 2, 3: ||t||^2, ||r0||^2, ||A r0||^2 of r0 = Z t;
//   4, 5, 6: ||r0||^2, ||g0||^2, ||A g0||^2 of g0 = Z r0   (idx < 0: quantity is 0)
// Writes rt_g = ||g0||^2, tol (tol_in, or the default rule :529-530 when tol_in is NaN), the
// radius, the orthogonality threshold -- and stop code 9 when the host must take over: a
// projection that needs refinement (projections.py:72-78) or the cancellation step
// (projector.null_space), or no room to the trust-region boundary (:515-526).
// taken (may be NULL): taken[pj] != 0 when projection pj already had its one correction step on
// the device (ipx_cg_prime: k_prime_decide) -- like the host's loop after its first step
// (projector.null_space, k >= 1) only the orthogonality test then stands.
// rguard (may be NULL): the radius guard's words X, Q, T (ipx_cg_args.rguard) -- X0 >= ||x0||
// from the reduction slot of ||x0||^2 (0 without one), Q0 >= ||p0|| = ||g0|| from rt_g, T = 0.
__device__ void prime_state_body(double *st, const double *red, const ipx_prime_idx &ix,
                                 double tol_in, double radius, double orth_tol, double norm_A,
                                 double canc2, const double *taken = nullptr,
                                 double *rguard = nullptr) {
  double q[7];
  for (int k = 0; k < 7; ++k) q[k] = ix.i[k] >= 0 ? red[ix.i[k]] : 0.0;
  bool bad = false;
  double margin = HUGE_VAL;
  for (int pj = 0; pj < 2; ++pj) {
    const double nx2 = q[1 + 3 * pj], nz2 = q[2 + 3 * pj], naz2 = q[3 + 3 * pj];
    const double nz = sqrt(nz2), naz = sqrt(naz2);
    const double orth = (nz == 0.0 || norm_A == 0.0) ? 0.0 : naz / (norm_A * nz);
    const bool stepped = taken && taken[pj] != 0.0;
    if (orth > orth_tol || (!stepped && nz2 < canc2 * nx2)) bad = true;
    if (!stepped && nx2 > 0.0) margin = fmin(margin, nz2 / nx2);
  }
  const double rt_g = q[5];
  const double tr_distance = radius - sqrt(q[0]);
  if (!(tr_distance >= 1e-25)) bad = true;
  double tol = tol_in;
  if (tol_in != tol_in) tol = fmax(fmin(0.01 * sqrt(rt_g), 0.1 * rt_g), 1e-25);
  for (int k = 0; k < ST_SIZE; ++k) st[k] = 0.0;
  st[ST_RTG0] = rt_g;
  st[ST_TOL] = tol;
  st[ST_RADIUS] = radius;
  st[ST_ORTH_RHS] = orth_tol * norm_A;
  st[ST_MARGIN] = margin;
  st[ST_PRIME_STEPS] = taken ? taken[0] + taken[1] : 0.0;
  st[ST_STOP] = bad ? 9.0 : 0.0;
  if (rguard) {
    rguard[IPX_RG_X] = ipx_rguard::start(q[0]);
    rguard[IPX_RG_Q] = ipx_rguard::start(rt_g);
    rguard[IPX_RG_T] = 0.0;
  }
}

__global__ void k_cg_prime_state(double *st, const double *__restrict__ red, ipx_prime_idx ix,
                                 double tol_in, double radius, double orth_tol, double norm_A,
                                 double canc2, double *rguard) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  prime_state_body(st, red, ix, tol_in, radius, orth_tol, norm_A, canc2, nullptr, rguard);
}

// The same behind the folds of the priming's SpMV partials (ipx_cg_prime: up to six products
// leave per-tile partials in separate regions of the workspace; folded here by the fold
// kernel's own routine, in its order, instead of by six launches of it)
struct PrimeFolds {
  const double *part[6];
  int count[6], slot[6], n;
  int single[6];            // 1: ONE sum per entry (the fused solve's tail), not the SpMV's pair
};
// radius_dev / norm_A2_dev (optional): the trust radius and ||A||_F^2 as DEVICE scalars that
// kernels earlier in the stream have written -- the outer iteration's chain (csrc/sqp.hip), whose
// tangential radius sqrt(Delta^2 - ||dn||^2) never visits the host.
// The correction step of a projection on the device (ipx_cg_prime).  After z = x - A'(A A')^-1 A x
// and t = A z, k_prime_decide folds their partials into red[base], red[base + 2] and decides
// what the host's loop decides from the same numbers (projector.null_space: orthogonality above
// the tolerance, or z cancelled below 2^-10 |x|): red[PR_SKIP + pj] = 0 lets the three guarded
// launches behind it run -- v = (A A')^-1 t, z <- z - A'v, t = A z -- whose partials (cz, ct) the
// NEXT decide kernel (or the state kernel) folds over red[base], red[base + 2]; taken:
// red[PR_TAKEN + pj] = 1.  One step per projection; what it does not settle is the host's (9).
#define PR_SKIP 14
#define PR_TAKEN 16
struct PrimeStep {          // one projection's correction: where its partials wait
  const double *cz, *ct;    // partials of the corrected ||z||^2 / of ||A z||^2
  int ncz, nct, base, pj;
  int pairs;                // 1: SpMV epilogue arrays [sum y^2 | sum x y]; 0: one sum each (the
                            // fused solve's tail: ||z||^2 per workgroup, residual partials)
};
__device__ void prime_fold4(const double *pz, int npz, const double *pt, int npt, int pairs,
                            double *lds, double (&out)[4]) {
  const double *parts[4] = {pz, pairs ? pz + npz : pz, pt, pairs ? pt + npt : pt};
  const int counts[4] = {npz, pairs ? npz : 0, npt, pairs ? npt : 0};
  ipx_sum_partials_multi<4>(parts, counts, lds, out);
}
__device__ void prime_fold_step(double *red, const PrimeStep &c, double *lds) {
  // (uniform across the block: red[PR_SKIP + pj] was written by an earlier kernel)
  if (red[PR_SKIP + c.pj] != 0.0) return;
  double out[4];
  prime_fold4(c.cz, c.ncz, c.ct, c.nct, c.pairs, lds, out);
  if (threadIdx.x == 0) {
    red[c.base] = out[0]; red[c.base + 1] = out[1];
    red[c.base + 2] = out[2]; red[c.base + 3] = out[3];
    red[PR_TAKEN + c.pj] = 1.0;
  }
  __syncthreads();
}
__global__ void __launch_bounds__(IPX_BLOCK)
k_prime_decide(double *red, const double *pz, int npz, const double *pt, int npt, int pairs,
               int base, int xslot, int pj, double orth_tol, double norm_A, double canc2,
               const double *__restrict__ norm_A2_dev, PrimeStep prev, int have_prev) {
  __shared__ double lds[4 * (IPX_BLOCK / IPX_WAVE)];
  if (have_prev) prime_fold_step(red, prev, lds);       // (||x||^2 of this projection: red[xslot])
  if (norm_A2_dev) norm_A = sqrt(*norm_A2_dev);
  double out[4];
  prime_fold4(pz, npz, pt, npt, pairs, lds, out);
  if (threadIdx.x != 0) return;
  red[base] = out[0]; red[base + 1] = out[1];
  red[base + 2] = out[2]; red[base + 3] = out[3];
  const double nx2 = red[xslot], nz2 = out[0], naz2 = out[2];
  const double nz = sqrt(nz2), naz = sqrt(naz2);
  const double orth = (nz == 0.0 || norm_A == 0.0) ? 0.0 : naz / (norm_A * nz);
  const bool need = orth > orth_tol || nz2 < canc2 * nx2;
  red[PR_SKIP + pj] = need ? 0.0 : 1.0;
  red[PR_TAKEN + pj] = 0.0;
}

__global__ void __launch_bounds__(IPX_BLOCK)
k_cg_prime_state_folds(double *st, double *red, PrimeFolds f, ipx_prime_idx ix, double tol_in,
                       double radius, double orth_tol, double norm_A, double canc2,
                       const double *__restrict__ radius_dev,
                       const double *__restrict__ norm_A2_dev, PrimeStep last, int have_last,
                       double *rguard) {
  if (radius_dev) radius = *radius_dev;
  if (norm_A2_dev) norm_A = sqrt(*norm_A2_dev);
  // all twelve sums (six jobs x [sum y^2 | sum x y]) in one pass: the loads of every array in
  // flight together, one barrier pair (one after the other: 12 us at n = 1e6; ~3 us this way);
  // the fold kernel's routine and order per array
  __shared__ double lds[12 * (IPX_BLOCK / IPX_WAVE)];
  const double *parts[12];
  int counts[12];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const bool on = j < f.n, two = on && !f.single[j];
    parts[2 * j] = on ? f.part[j] : f.part[0];
    parts[2 * j + 1] = two ? f.part[j] + f.count[j] : f.part[0];
    counts[2 * j] = on ? f.count[j] : 0;
    counts[2 * j + 1] = two ? f.count[j] : 0;
  }
  double out[12];
  if (f.n > 0) {
    ipx_sum_partials_multi<12>(parts, counts, lds, out);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int j = 0; j < 6; ++j)
        if (j < f.n) { red[f.slot[j]] = out[2 * j]; red[f.slot[j] + 1] = out[2 * j + 1]; }
    }
    __syncthreads();
  }
  if (have_last) prime_fold_step(red, last, lds);
  // (thread 0 reads back what it wrote itself)
  if (threadIdx.x == 0)
    prime_state_body(st, red, ix, tol_in, radius, orth_tol, norm_A, canc2,
                     have_last ? red + PR_TAKEN : nullptr, rguard);
}

int ipx_cg_prime_state_guard(double *state, const double *red, const int32_t *idx7,
                             double tol_in, double radius, double orth_tol, double norm_A,
                             double cancellation, double *rguard, void *stream) {
  if (!state || !red || !idx7) return IPX_EINVAL;
  ipx_prime_idx ix;
  for (int k = 0; k < 7; ++k) ix.i[k] = idx7[k];
  hipLaunchKernelGGL(k_cg_prime_state, dim3(1), dim3(64), 0, (hipStream_t)stream, state, red, ix,
                     tol_in, radius, orth_tol, norm_A, cancellation * cancellation, rguard);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

int ipx_cg_prime_state(double *state, const double *red, const int32_t *idx7, double tol_in,
                       double radius, double orth_tol, double norm_A, double cancellation,
                       void *stream) {
  return ipx_cg_prime_state_guard(state, red, idx7, tol_in, radius, orth_tol, norm_A, cancellation,
                                  nullptr, stream);
}

// The whole priming of a projected_cg call (qp_subproblem.py:502-512) behind ONE entry point:
//   x0 = Y(-b) = A'(A A')^-1(-b)            (b == NULL: b = 0, x0 = 0)
//   t  = H x0 + c;   r0 = Z t;   g0 = Z r0  (Z v = v - A'(A A')^-1 A v, each with ||v||^2,
//                                            ||Z v||^2 and ||A Z v||^2 left in `red`)
//   the state block (ipx_cg_prime_state);   p = -g0;   Hp = H p
// into the loop's own buffers (x0 -> a->x, r0 -> a->r, p -> a->p; a->Hp, a->w, a->v, a->t as
// scratch): the kernels and their order are those the Python host enqueued one ctypes call at
// a time (ipsolver/projector.py null_space_enqueue), ~25 calls and three copies.  CSR A and H
// (+ optional diagonal), banded or box-Schur solver; red: >= 14 doubles of device memory, ws:
// the reduction workspace (IPX_WS_DOUBLES).
static int prime_solve(const ipx_cg_args *a, const double *w, double *v, void *stream) {
  if (a->solver_kind == 1)
    return ipx_boxschur_solve((const ipx_boxschur_args *)a->banded, w, v, nullptr, nullptr, nullptr,
                              stream);
  return ipx_banded_solve(a->banded, w, v, stream);
}
// The priming's products with a norm: per-tile partials into the next free region of the
// workspace, folded later by k_cg_prime_state_folds.
struct PrimeRed {
  double *red, *ws;
  int64_t off;
  PrimeFolds f;
  int spmv(const ipx_csr_view &M, const double *x, double alpha, const double *diag, double beta,
           const double *yin, double *yout, int slot, hipStream_t st) {
    double *part = ws + off;
    off += 2 * (int64_t)M.ntiles;
    f.part[f.n] = part; f.count[f.n] = M.ntiles; f.slot[f.n] = slot; f.single[f.n] = 0; ++f.n;
    return ipx_spmv_launch(M, x, alpha, diag, beta, yin, yout, part, nullptr, st);
  }
  void single(const double *part, int count, int slot) {
    f.part[f.n] = part; f.count[f.n] = count; f.slot[f.n] = slot; f.single[f.n] = 1; ++f.n;
  }
};

// z = sign (x - A'(A A')^-1 A x) with ||z||^2 -> red[base], ||A z||^2 -> red[base + 2] and,
// unless the caller has it already (have_xnorm), ||x||^2 -> red[base + 4].  sign = -1 writes
// the negated projection by the same roundings (alpha, beta = 1, -1 instead of -1, 1: a
// difference and its negation round alike), the norms do not see the sign.
static int prime_project(const ipx_cg_args *a, const ipx_csr_view &A, const ipx_csr_view &At,
                         const double *x, double *z, PrimeRed &R, int base, bool have_xnorm,
                         double sign, hipStream_t st) {
  int rc = have_xnorm ? IPX_OK : ipx_norms(a->n, x, R.red + base + 4, R.ws + R.off, st);
  if (rc) return rc;
  rc = ipx_spmv_launch(A, x, 1.0, nullptr, 0.0, nullptr, a->w, nullptr, nullptr, st);
  if (rc) return rc;
  rc = prime_solve(a, a->w, a->v, st);
  if (rc) return rc;
  rc = R.spmv(At, a->v, -sign, nullptr, sign, x, z, base, st);
  if (rc) return rc;
  return R.spmv(A, z, 1.0, nullptr, 0.0, nullptr, a->t, base + 2, st);
}

// The same projection through the loop's own second launch (tridiagonal A A' on the cyclic-
// reduction / decoupled solve with g = r - A'v as its tail: csrc/banded.hip AtvJob): w = A x by
// the SpMV, then ONE launch for v = (A A')^-1 w, z = sign (x - A'v), the per-workgroup partials
// of ||z||^2 (pz) and of ||w - (A A') v||^2 = ||A z||^2 (pt: the orthogonality measure the
// loop's iterations use, projections.py:52 without a second product by A) -- two launches
// instead of four.  guard: *guard != 0 skips both (a correction step that is not due).
// Under PJ_STEP1_SOLVE_TAIL both are ONE launch, the loop's fused projection without its step
// (k_step1_solve_tail<.., PRIME>) -- where z is not x: a workgroup reads x on its whole window.
static int prime_project_tail(const ipx_cg_args *a, const LoopPlan &P, const ipx_csr_view &A,
                              const double *x, double *z, double *pz, double *pt, int *np,
                              double sign, const double *guard, hipStream_t st) {
  if (P.proj == PJ_STEP1_SOLVE_TAIL && x != z) {
    ipx_fused_proj_job J{};
    J.r_in = x; J.g_out = z; J.xn = 1; J.prime = 1; J.sign = sign; J.guard = guard;
    J.A_ell_val = a->A_ell_val; J.A_ell_off16 = (const uint16_t *)a->A_ell_off16;
    J.contig = a->A_contig != 0;
    J.A_rowfirst = a->A_rowfirst; J.rl = (int)a->A_rl; J.win = a->P_win; J.n = a->n;
    J.vown = a->At_vown; J.qv = (int)a->At_qv; J.ell_row = a->At_ell_row; J.ell_val = a->At_ell_val;
    J.v = a->v; J.part3 = pz; J.part4 = pt;
    return ipx_banded_fused_proj_launch(a->banded, J, np, st);
  }
  int rc = ipx_spmv_launch(A, x, 1.0, nullptr, 0.0, nullptr, a->w, nullptr, guard, st);
  if (rc) return rc;
  return ipx_banded_solve_resid_atv_launch(a->banded, a->w, a->v, pt, np, a->At_rowptr,
                                           a->At_colidx, a->At_val, x, z, a->At_vown,
                                           (int)a->At_qv, pz, guard, st, a->At_ell_row,
                                           a->At_ell_val, a->n, sign);
}

// either way, the partials registered for the state kernel's fold
static int prime_project_any(const ipx_cg_args *a, const LoopPlan &P, const ipx_csr_view &A,
                             const ipx_csr_view &At, const double *x, double *z, PrimeRed &R,
                             int base, bool have_xnorm, double sign, hipStream_t st) {
  // (PJ_STEP1_SOLVE_TAIL: the priming's projections are the solve-with-tail pair all the same)
  if (P.proj != PJ_SOLVE_TAIL && P.proj != PJ_STEP1_SOLVE_TAIL)
    return prime_project(a, A, At, x, z, R, base, have_xnorm, sign, st);
  int rc = have_xnorm ? IPX_OK : ipx_norms(a->n, x, R.red + base + 4, R.ws + R.off, st);
  if (rc) return rc;
  const int cap = (int)((a->m + 255) / 256) + 8;
  double *pz = R.ws + R.off, *pt = pz + 2 * cap;
  R.off += 3 * (int64_t)cap;
  int np = 0;
  rc = prime_project_tail(a, P, A, x, z, pz, pt, &np, sign, nullptr, st);
  if (rc) return rc;
  R.single(pz, np, base);
  R.single(pt, np, base + 2);
  return IPX_OK;
}

// ... and with its correction step decided and taken on the device (k_prime_decide): the
// projection's own partials are folded by the decide kernel (they leave R.f), the step's wait in
// two more regions for the next decide / the state kernel (`step` out; `prev`: the projection
// before this one, whose step this decide kernel folds first).  z - A'v' with v' = (A A')^-1 A z
// is the same expression for z and for -z (every launch an odd function of its input, bit for
// bit), so the negated second projection needs no sign.
static int prime_project_stepped(const ipx_cg_args *a, const LoopPlan &P,
                                 const ipx_csr_view &A, const ipx_csr_view &At, const double *x, double *z, PrimeRed &R,
                                 int base, int xslot, int pj, bool have_xnorm, double sign,
                                 double orth_tol, double norm_A, const double *norm_A2_dev,
                                 double canc2, const PrimeStep *prev, PrimeStep *step,
                                 hipStream_t st) {
  const int n0 = R.f.n;
  int rc;
  const double *skip = R.red + PR_SKIP + pj;
  if (P.proj == PJ_SOLVE_TAIL || P.proj == PJ_STEP1_SOLVE_TAIL) {
    if (!have_xnorm) {
      rc = ipx_norms(a->n, x, R.red + base + 4, R.ws + R.off, st);
      if (rc) return rc;
    }
    const int cap = (int)((a->m + 255) / 256) + 8;      // (>= workgroups of the solve, twice)
    double *pz = R.ws + R.off, *pt = pz + 2 * cap, *cz = pt + cap, *ct = cz + 2 * cap;
    R.off += 6 * (int64_t)cap;
    int np = 0, npc = 0;
    rc = prime_project_tail(a, P, A, x, z, pz, pt, &np, sign, nullptr, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_prime_decide, dim3(1), dim3(IPX_BLOCK), 0, st, R.red, pz, np, pt, np, 0,
                       base, xslot, pj, orth_tol, norm_A, canc2, norm_A2_dev,
                       prev ? *prev : PrimeStep{}, prev ? 1 : 0);
    IPX_CHECK_LAUNCH();
    // the step: z <- z - A'(A A')^-1 (A z), the same two launches on z itself (in place: the
    // tail reads and writes one variable per lane), guarded
    rc = prime_project_tail(a, P, A, z, z, cz, ct, &npc, 1.0, skip, st);
    if (rc) return rc;
    *step = PrimeStep{cz, ct, npc, npc, base, pj, 0};
    return IPX_OK;
  }
  rc = prime_project(a, A, At, x, z, R, base, have_xnorm, sign, st);
  if (rc) return rc;
  // (the two regions this projection just registered: folded here, not by the state kernel)
  const double *pz = R.f.part[n0], *pt = R.f.part[n0 + 1];
  const int npz = R.f.count[n0], npt = R.f.count[n0 + 1];
  R.f.n = n0;
  hipLaunchKernelGGL(k_prime_decide, dim3(1), dim3(IPX_BLOCK), 0, st, R.red, pz, npz, pt, npt, 1,
                     base, xslot, pj, orth_tol, norm_A, canc2, norm_A2_dev,
                     prev ? *prev : PrimeStep{}, prev ? 1 : 0);
  IPX_CHECK_LAUNCH();
  if (a->solver_kind == 1)
    rc = ipx_boxschur_solve((const ipx_boxschur_args *)a->banded, a->t, a->v, nullptr, nullptr, skip,
                            st);
  else
    rc = ipx_banded_solve_guarded(a->banded, a->t, a->v, skip, st);
  if (rc) return rc;
  double *cz = R.ws + R.off;
  R.off += 2 * (int64_t)At.ntiles;
  double *ct = R.ws + R.off;
  R.off += 2 * (int64_t)A.ntiles;
  rc = ipx_spmv_launch(At, a->v, -1.0, nullptr, 1.0, z, z, cz, skip, st);
  if (rc) return rc;
  rc = ipx_spmv_launch(A, z, 1.0, nullptr, 0.0, nullptr, a->t, ct, skip, st);
  if (rc) return rc;
  *step = PrimeStep{cz, ct, At.ntiles, A.ntiles, base, pj, 1};
  return IPX_OK;
}

int64_t ipx_cg_prime_ws_doubles(const ipx_cg_args *a, int32_t A_ntiles) {
  if (!a) return -1;
  // (three products by A', two by A, one by H; + the two correction steps' A' and A products)
  return 2 * (5 * a->At_ntiles + 4 * (int64_t)A_ntiles + a->H_ntiles) + 4096;
}

int ipx_cg_prime(const ipx_cg_args *a, const int32_t *A_tiles, int32_t A_ntiles, const double *c,
                 const double *b, double *red, double *ws, double tol_in, double radius,
                 double orth_tol, double norm_A, double cancellation, int32_t first_end,
                 int32_t steps, void *stream) {
  return ipx_cg_prime_dev(a, A_tiles, A_ntiles, c, b, red, ws, tol_in, radius, nullptr, orth_tol,
                          norm_A, nullptr, cancellation, first_end, steps, nullptr, 0, 0,
                          (hipStream_t)stream);
}

}  // extern "C"

int ipx_cg_prime_dev(const ipx_cg_args *a, const int32_t *A_tiles, int32_t A_ntiles,
                     const double *c, const double *b, double *red, double *ws, double tol_in,
                     double radius, const double *radius_dev, double orth_tol, double norm_A,
                     const double *norm_A2_dev, double cancellation, int32_t first_end,
                     int steps, const double *c_part, int32_t c_npart, int x_is_zero,
                     hipStream_t stream) {
  if (!a || !c || !red || !ws || !A_tiles || a->solver_kind > 1 || a->m <= 0 || a->H_operator ||
      !a->H_rowptr || !a->t || first_end < 0 || a->LR_W)   // (H x0 would miss a low-rank term)
    return IPX_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const LoopPlan P = plan_of(a);
  const ipx_csr_view A{(int)a->m, (int)a->n, a->A_rowptr, a->A_colidx, a->A_val, A_tiles, A_ntiles};
  const ipx_csr_view At{(int)a->n, (int)a->m, a->At_rowptr, a->At_colidx, a->At_val, a->At_tiles,
                        (int)a->At_ntiles};
  const ipx_csr_view Hm{(int)a->n, (int)a->n, a->H_rowptr, a->H_colidx, a->H_val, a->H_tiles,
                        (int)a->H_ntiles};
  // the products' norms come out of their epilogues (no norm kernels); their per-tile partials
  // wait in the workspace for ONE fold in front of the state kernel: six regions (n = 1e6: 17 k
  // of the 64 k doubles) and a 4096-double tail for ipx_norms.  A problem whose regions do not
  // fit (n beyond ~5e6 on the benchmark's band) is primed launch by launch by the caller.
  if (ipx_cg_prime_ws_doubles(a, A_ntiles) > IPX_WS_DOUBLES) return IPX_EUNSUPPORTED;
  PrimeRed R{red, ws, 0, PrimeFolds{}};
  int rc;
  const double *t = c;
  if (b) {
    // x0 = A'(A A')^-1 (-b) = -A' (A A')^-1 b: the solve and the product are odd functions of
    // their input down to the last bit, so the sign is applied by the product's scalar
    rc = prime_solve(a, b, a->v, stream);
    if (rc) return rc;
    rc = R.spmv(At, a->v, -1.0, nullptr, 0.0, nullptr, a->x, 12, st);
    if (rc) return rc;
    rc = R.spmv(Hm, a->x, 1.0, a->H_diag, 1.0, c, a->Hp, 4, st);
    if (rc) return rc;
    t = a->Hp;
  } else if (!x_is_zero &&
             hipMemsetAsync(a->x, 0, (size_t)a->n * sizeof(double), st) != hipSuccess) {
    return IPX_ELAUNCH;
  }
  const double canc2 = cancellation * cancellation;
  PrimeStep s1{}, s2{};
  if (b || !steps) {
    // (b: ||t||^2 = red[4] comes out of the H x0 + c product's partials, folded by the state
    // kernel: the first projection's decision would need it earlier -- no step on this path)
    const bool c_known = !b && c_part && c_npart > 0;
    if (c_known) {                 // (||c||^2 -> red[4]: folded by the state kernel)
      PrimeFolds &f = R.f;
      f.part[f.n] = c_part; f.count[f.n] = c_npart; f.slot[f.n] = 4; f.single[f.n] = 0; ++f.n;
    }
    rc = prime_project_any(a, P, A, At, t, a->r, R, 0, b != nullptr || c_known, 1.0, st);
    if (rc) return rc;
    rc = prime_project_any(a, P, A, At, a->r, a->p, R, 6, true, -1.0, st);
    if (rc) return rc;
  } else {
    rc = prime_project_stepped(a, P, A, At, t, a->r, R, 0, 4, 0, false, 1.0, orth_tol, norm_A,
                               norm_A2_dev, canc2, nullptr, &s1, st);
    if (rc) return rc;
    // g0 = Z r0 lands in p as -g0 (the first direction); its input norm ||r0||^2 is red[0]
    rc = prime_project_stepped(a, P, A, At, a->r, a->p, R, 6, 0, 1, true, -1.0, orth_tol, norm_A,
                               norm_A2_dev, canc2, &s1, &s2, st);
    if (rc) return rc;
  }
  const int32_t idx_b[7] = {12, 4, 0, 2, 0, 6, 8}, idx_0[7] = {-1, 4, 0, 2, 0, 6, 8};
  ipx_prime_idx ix;
  for (int k = 0; k < 7; ++k) ix.i[k] = (b ? idx_b : idx_0)[k];
  hipLaunchKernelGGL(k_cg_prime_state_folds, dim3(1), dim3(IPX_BLOCK), 0, st, a->state, red, R.f,
                     ix, tol_in, radius, orth_tol, norm_A, canc2, radius_dev, norm_A2_dev, s2,
                     (b || !steps) ? 0 : 1, a->radius_guard != 0 ? a->rguard : nullptr);
  IPX_CHECK_LAUNCH();
  rc = launch_hp(a, P, nullptr, st);
  if (rc || first_end == 0) return rc;
  // the call's first batch behind the same entry (stop code 9: its launches do nothing)
  return cg_iterate(a, P, 0, first_end, st, nullptr);
}

extern "C" {

// Hp = H p with p'Hp partials (the tail of an iteration, also used once by
// the host to prime the loop).
int ipx_cg_hp(const ipx_cg_args *a, void *stream) {
  if (!a) return IPX_EINVAL;
  return launch_hp(a, plan_of(a), nullptr, (hipStream_t)stream);
}

// The update half with the fused step2 + H.p kernel on its own (iteration `it`, step2 mode bits
// as in ipx_cg_resume), long partial arrays compacted first as in the loop; IPX_EINVAL when the
// argument block does not enable the kernel.
int ipx_cg_step2_hp(const ipx_cg_args *a, int32_t it, int32_t mode, void *stream) {
  if (!a || (mode & ~3)) return IPX_EINVAL;                   // (bit 4: ipx_cg_iterate's alone)
  LoopPlan P = plan_of(a);
  if (!P.fused_hp) return IPX_EINVAL;
  P.step2 = S2_FUSED_HP;
  Compactor cmp(a, nullptr);
  HalfArgs h{it, mode, a->state + ST_STOP};
  h.cmp = &cmp;
  return launch_update_half(a, P, h, a->part2, P.np2, a->part3, P.np3, a->part4, P.np4,
                            (hipStream_t)stream);
}

// Tail of an iteration after the host handled a stop-5 / stop-6 event: the update half with
// the given mode and step2 as the vector kernel, then Hp = H p.
int ipx_cg_resume(const ipx_cg_args *a, int32_t it, int32_t mode, void *stream) {
  if (!a) return IPX_EINVAL;
  LoopPlan P = plan_of(a);
  P.step2 = S2_VECTOR;
  const HalfArgs h{it, mode, a->state + ST_STOP};
  // the radius guard: the vector step2 moves x and p without the guard's kernel -- only behind a
  // test that was taken (mode bit 1: part2 holds nothing), and the bounds move with them
  if (P.guard && !(mode & 1)) return IPX_EINVAL;
  int rc = launch_update_half(a, P, h, a->part2, P.np2, a->part3, P.np3, a->part4, P.np4,
                              (hipStream_t)stream);
  if (rc || !P.guard) return rc;
  // (the H.p launches behind step2 leave the state block alone)
  hipLaunchKernelGGL(k_rguard_advance, dim3(1), dim3(1), 0, (hipStream_t)stream,
                     (const double *)a->state, it & 1, a->rguard);
  IPX_CHECK_LAUNCH();
  return IPX_OK;
}

// The radius guard lost on iteration it_stop (stop code 11, cleared by the caller): the sums the
// carried form would hold, then that iteration's update half in the carried form.
int ipx_cg_guard_resume(const ipx_cg_args *a, int32_t it_stop, void *stream) {
  if (!a || !a->xsums || !a->rguard) return IPX_EINVAL;
  LoopPlan P = plan_of(a);
  if (!P.xsums || P.step2 != S2_FUSED_HP) return IPX_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  double *comp = a->xsums + 3 * a->H_ntiles + 1;
  hipLaunchKernelGGL(k_rguard_sums, dim3(XS_STRIDE), dim3(IPX_BLOCK), 0, st, a->n,
                     (const double *)a->x, (const double *)a->p, comp);
  IPX_CHECK_LAUNCH();
  const double *guard = a->state + ST_STOP;
  Compactor cmp(a, guard);
  HalfArgs h{it_stop, 4, guard};
  h.cmp = &cmp;
  h.xs = ipx_xsums_job{a->xsums, comp, it_stop, 1};
  int rc = launch_update_half(a, P, h, a->part2, P.np2, a->part3, P.np3, a->part4, P.np4, st);
  if (rc) return rc;
  // the folded arrays as the loop's launches expect them: zeros behind the xs_ncomp entries the
  // projection half of the next carried iteration writes
  if (hipMemsetAsync(comp, 0, (size_t)3 * XS_STRIDE * sizeof(double), st) != hipSuccess)
    return IPX_ELAUNCH;
  return IPX_OK;
}

double ipx_rguard_start(double sumsq) { return ipx_rguard::start(sumsq); }
double ipx_rguard_step_x(double X, double Q, double alpha) {
  return ipx_rguard::step_x(X, Q, alpha);
}
double ipx_rguard_step_q(double Q, double beta, double gg) {
  return ipx_rguard::step_q(Q, beta, gg);
}

int ipx_cg_iterate(const ipx_cg_args *a, int32_t it_begin, int32_t it_end, void *stream) {
  if (!a || it_end < it_begin) return IPX_EINVAL;
  return cg_iterate(a, plan_of(a), it_begin, it_end, (hipStream_t)stream, nullptr);
}

// Instrumented variant for bench.py: HIP events are recorded on `stream`
// around every kernel class of every iteration; after one final stream
// synchronise the per-class totals (ms) are returned in ms_out[0..6]:
// step1, spmv A r, banded solve, spmv r-A'v, spmv A g, step2, spmv H p.
// Slower than ipx_cg_iterate (event records between kernels) -- use it for
// per-kernel attribution, not for the throughput number.
// Under the fused projection (PJ_STEP1_SOLVE_TAIL) the one launch of the projection half is
// booked under "banded solve" (the classes before and behind it read 0).  The iterations are
// enqueued one cg_iterate call each, so every one of them ends with the guarded copy
// k_cg_settle_r moving r_next back into r (8 n bytes each way) -- behind the iteration's last
// event and before the next one's first: in no class, but in the wall clock of this entry;
// the batch loop launches it once per call and copies only after an odd count.
#define IPX_CG_NCLASS 7
int ipx_cg_iterate_timed(const ipx_cg_args *a, int32_t it_begin, int32_t it_end, float *ms_out,
                         void *stream) {
  if (!a || it_end < it_begin || !ms_out) return IPX_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const LoopPlan P = plan_of(a);
  const int per_it = IPX_CG_NCLASS + 1;
  const int nit = it_end - it_begin;
  std::vector<hipEvent_t> ev((size_t)nit * per_it);
  for (auto &e : ev)
    if (hipEventCreate(&e) != hipSuccess) return IPX_ELAUNCH;
  int rc = IPX_OK;
  for (int i = 0; i < nit && rc == IPX_OK; ++i)
    rc = cg_iterate(a, P, it_begin + i, it_begin + i + 1, st, ev.data() + (size_t)i * per_it);
  if (hipStreamSynchronize(st) != hipSuccess) rc = IPX_ELAUNCH;
  for (int c = 0; c < IPX_CG_NCLASS; ++c) ms_out[c] = 0.f;
  if (rc == IPX_OK) {
    for (int i = 0; i < nit; ++i)
      for (int c = 0; c < IPX_CG_NCLASS; ++c) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ev[(size_t)i * per_it + c], ev[(size_t)i * per_it + c + 1]);
        ms_out[c] += ms;
      }
  }
  for (auto &e : ev) (void)hipEventDestroy(e);
  return rc;
}

}  // extern "C"
