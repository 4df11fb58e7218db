"""Every solve with S = A A' judged by an exact residual (tests/normal_ref.py).

A is an integer matrix whose rows are scaled by powers of two, so S is exactly representable
and the device assembles it exactly; the residual r = w - S v of a computed v is evaluated
correctly rounded, and v is judged by the normwise backward error of the diagonally scaled
system, eta = ||D^-1 r|| / (||D^-1 S D^-1|| ||D v|| + ||D^-1 w||) (infinity norms, D = diag of
powers of two near sqrt(S_ii)): a number that row scaling changes only through rounding.

Paths, on the same matrix wherever they apply: ipx_banded_solve (whichever form the
factorization chose), ipx_banded_solve_resid, ipx_banded_solve_multilaunch, the full path
(ipx_banded_set_decoupling 0), the chunk form of the single-launch solve (2), the box-Schur
elimination, the dense Cholesky + explicit inverse, and the preconditioned CG (block, jacobi).

Bounds (u = 2^-53).  Direct banded forms: a banded LDL' (chunks, separators, the cyclic
reduction, all fixed-order fp64) is backward stable, |dS| <= gamma_{c(k+1)} |L||D||L'|, and in
the scaled norms |L||D||L'| is O(k+1) times ||D^-1 S D^-1||; the decoupling decisions drop
couplings below 2^-56 = u/8 of the smaller diagonal entry they touch, the cyclic reduction's
reciprocal (v_rcp_f64 + one Newton step) is correctly rounded to within an ulp.  So
eta <= C_DIRECT (k + 1) u, C_DIRECT a small constant.  Defect correction stops at
eta_c^(N+1) <= 2^-54 (eta_c the measured contraction bound, < 0.5): its own constant
C_ITER (k + 1) u, the N correction steps adding one rounding of the residual each.  The dense
path applies an explicit inverse (not backward stable): eta <= C_DENSE m u kappa(D^-1 S D^-1).
The CG: its own stopping rule, ||r||_2 <= WARN_RELRES ||w||_2 (IterativeNormalSolver).
The constants were set from the largest eta / u measured per path (printed by the tests), with
the margin stated next to them.
"""
import ctypes
import math
import warnings

import numpy as np
import pytest
import scipy.sparse as sps

import normal_ref as nr

pytestmark = pytest.mark.gpu

U = nr.U
IPX_OK, IPX_EUNSUPPORTED, IPX_EILLCOND = 0, -5, -6

# largest eta / u measured on an MI355X over every family and shape (printed by the tests):
C_DIRECT = 4.0       # 1.55 (k = 1, the L = 7 edge): bound 4 (k + 1) u >= 8 u, margin >= 5x
C_ITER = 8.0         # defect correction (k = 5, 6; 42 / 45 steps): within the direct maxima
C_BOX = 8.0          # box-Schur: the banded solve of the Schur complement + the closed forms
C_DENSE = 1.0        # dense: eta <= C m u kappa; measured 8e-4 m u kappa

# The CG (IterativeNormalSolver) is judged by its own stopping rule on the true residual:
#   ||r||_2 <= tol ||w||_2 + C_CG u || |S||v| + |w| ||_2,
# tol = 10 RTOL when it declared convergence (its recurrence residual below RTOL ||w||), else
# WARN_RELRES.  The second term is the rounding floor of w - S v itself: with graded rows
# ||S|| ||v|| can exceed ||w|| by 2^60, and then even the correctly rounded S^-1 w has an
# unscaled residual above ||w|| (its scaled backward error stays ~u).
C_CG = 16.0          # measured: at most 2.4 past tol ||w|| (graded rows); margin ~7x

SEEN = {}


def _seen(path, family, value):
    key = (path, family)
    SEEN[key] = max(SEEN.get(key, 0.0), value)
    print("eta/u %-12s %-22s %.3g" % (path, family, value))


@pytest.fixture(scope="module")
def env():
    import torch
    from ipsolver import _hip, device as dv, projector

    class NS:
        pass
    ns = NS()
    ns.torch, ns.hip, ns.dv, ns.proj, ns.lib = torch, _hip, dv, projector, _hip.load()
    yield ns
    for key in sorted(SEEN):
        print("largest eta/u %-12s %-22s %.3g" % (key + (SEEN[key],)))


# ---------------------------------------------------------------------- matrix families
def _csr(vals, rows, cols, shape):
    A = sps.csr_matrix((np.asarray(vals, dtype=np.float64), (rows, cols)), shape=shape)
    A.sort_indices()
    return A


def band_rows(rng, m, k, lim=2 ** 10, private=False):
    """(a) Random integer rows over columns 3i .. 3i + 3k: A A' of half bandwidth exactly k,
    well conditioned (rows of 3k + 1 random entries, neighbours sharing a third of them).
    ``private``: plus an entry in [2^11, 2^12) on a column of its own -- a diagonally dominant
    S, whose inverse decays fast enough for the chunk separators to decouple at any k."""
    w = 3 * k + 1
    cols = (3 * np.arange(m)[:, None] + np.arange(w)[None, :]).ravel()
    rows, vals, n = np.repeat(np.arange(m), w), nr.int_values(rng, m * w, lim), 3 * m + 3 * k + 1
    if private:
        rows = np.concatenate((rows, np.arange(m)))
        cols = np.concatenate((cols, n + np.arange(m)))
        vals = np.concatenate((vals, rng.integers(2 ** 11, 2 ** 12, m).astype(np.float64)))
        n += m
    return _csr(vals, rows, cols, (m, n))


def moving_average(m, k, W, eps, rng=None, noise=0):
    """(c)/(d) Row i: weight W (+ integer noise) on columns i .. i + k and eps on a private
    column: S = triangle-kernel Toeplitz + eps^2 I, nearly dependent neighbours for eps << W
    (cond ~ ((k + 1) W / eps)^2), half bandwidth k."""
    vals = np.full((m, k + 1), W, dtype=np.int64)
    if noise:
        vals = vals + rng.integers(-noise, noise + 1, (m, k + 1))
    cols = (np.arange(m)[:, None] + np.arange(k + 1)[None, :]).ravel()
    rows = np.repeat(np.arange(m), k + 1)
    return _csr(np.concatenate((vals.ravel(), np.full(m, eps))),
                np.concatenate((rows, np.arange(m))),
                np.concatenate((cols, m + k + np.arange(m))), (m, 2 * m + k))


def ramp_blocks(nblocks, size=31, eps=7):
    """Tridiagonal blocks of ``size`` rows that share no column with each other (row i: 1, 1 on
    two consecutive columns, eps on a private one: coupling ratio 1 / (2 + eps^2), the
    reduction decouples at distance 16), with the rows of each block to be scaled by
    2^(2l - 30), l = 0 .. size - 1: a steep ramp along the band."""
    m = nblocks * size
    i = np.arange(m)
    b, l = i // size, i % size
    c0 = b * (size + 1) + l
    A = _csr(np.concatenate((np.ones(2 * m), np.full(m, eps))),
             np.concatenate((i, i, i)),
             np.concatenate((c0, c0 + 1, nblocks * (size + 1) + i)),
             (m, nblocks * (size + 1) + m))
    return A, 2 * l - 30


# ----------------------------------------------------------------------------- runners
def _h(solver):
    return ctypes.c_void_p(solver.handle)


def _decisions(lib, h):
    eta = ctypes.c_double(0.0)
    steps = lib.ipx_banded_refine_steps(h, ctypes.byref(eta))
    return {"decoupled": int(lib.ipx_banded_decoupled(h)), "L": int(lib.ipx_banded_pcr_level(h)),
            "steps": int(steps), "eta": float(eta.value)}


def _geometry(lib, h):
    geo = (ctypes.c_int32 * 2)()
    return (int(geo[0]), int(geo[1])) if lib.ipx_banded_decoupled_geometry(h, geo) else None


class Banded:
    """A BandedNormalSolver on A and every form of its solve, outputs on the host."""

    def __init__(self, env, A):
        self.env, self.A = env, A
        self.m = A.shape[0]
        self.solver = env.proj.BandedNormalSolver(env.dv.DeviceCSR.from_scipy(A))
        assert self.solver.perm is None
        self.k = self.solver.k
        self.h = _h(self.solver)
        lib = env.lib
        self.dec = _decisions(lib, self.h)
        self.geo = _geometry(lib, self.h)
        self.dec["status"] = int(lib.ipx_banded_status(self.h, env.dv.stream_ptr()))
        assert _decisions(lib, self.h) == {k: v for k, v in self.dec.items() if k != "status"}
        # half bandwidths 5..8 past 2048 rows have no compiled separator level (ipx_banded_create)
        self.wide = self.k >= 5 and self.m > 2048

    def _vec(self, fill=float("nan")):
        t = self.env.torch
        return t.full((self.m,), fill, dtype=t.float64, device="cuda")

    def _call(self, name, wd, x, *extra):
        env = self.env
        rc = getattr(env.lib, name)(self.h, env.dv._p(wd), env.dv._p(x), *extra,
                                    env.dv.stream_ptr())
        return rc

    def run(self, w):
        """{path: x} for every form that applies, and the resid form's partial sums."""
        env, lib, torch = self.env, self.env.lib, self.env.torch
        wd = torch.from_numpy(np.ascontiguousarray(w)).cuda()
        out = {}
        x = self._vec()
        assert self._call("ipx_banded_solve", wd, x) == IPX_OK
        out["solve"] = x.cpu().numpy()
        x = self._vec()
        part = torch.full((self.m // 256 + 2,), float("nan"), dtype=torch.float64, device="cuda")
        npart = ctypes.c_int32(0)
        env.hip.call("ipx_banded_solve_resid", self.h, env.dv._p(wd), env.dv._p(x),
                     env.dv._p(part), ctypes.byref(npart), None, env.dv.stream_ptr())
        out["resid"] = x.cpu().numpy()
        p = part.cpu().numpy()
        assert 1 <= npart.value <= len(p) and not np.isnan(p[:npart.value]).any()
        self.partials = p[:npart.value]
        x = self._vec()
        rc = self._call("ipx_banded_solve_multilaunch", wd, x)
        if self.wide:
            assert rc == IPX_EUNSUPPORTED
        else:
            assert rc == IPX_OK
            out["multilaunch"] = x.cpu().numpy()
        if self.dec["decoupled"] and self.dec["L"] > 2:
            # the reduction forced to stop two levels early: an inexact solve, whose fused
            # residual must still be the residual of what it returned
            lib.ipx_banded_set_decoupling(self.h, 16 + self.dec["L"] - 2)
            x = self._vec()
            env.hip.call("ipx_banded_solve_resid", self.h, env.dv._p(wd), env.dv._p(x),
                         env.dv._p(part), ctypes.byref(npart), None, env.dv.stream_ptr())
            self.early = (x.cpu().numpy(), part.cpu().numpy()[:npart.value])
            lib.ipx_banded_set_decoupling(self.h, 16 + self.dec["L"])
        if self.dec["decoupled"]:
            lib.ipx_banded_set_decoupling(self.h, 2)           # the chunk form
            x = self._vec()
            assert self._call("ipx_banded_solve", wd, x) == IPX_OK
            out["chunk"] = x.cpu().numpy()
        lib.ipx_banded_set_decoupling(self.h, 0)               # the full path
        x = self._vec()
        rc = self._call("ipx_banded_solve", wd, x)
        if self.wide and self.dec["steps"] == 0:
            assert rc == IPX_EUNSUPPORTED
        else:
            assert rc == IPX_OK
            out["full"] = x.cpu().numpy()
        return out


def _direct_bound(k, steps):
    return (C_ITER if steps else C_DIRECT) * (k + 1) * U


def check_banded(env, A, e, w, family, S=None, expect_status=IPX_OK):
    """All banded forms on diag(2^e) A: eta within the bound, the resid form's x bit-identical
    to the plain solve's, its partials the squared norm of fl(w - S x)."""
    Ae = nr.pow2_rows(A, e)
    S = nr.gram_pow2(A, e) if S is None else S
    b = Banded(env, Ae)
    assert b.dec["status"] == expect_status, b.dec
    outs = b.run(w)
    assert np.array_equal(outs["resid"], outs["solve"])
    k = b.k
    r_solve = None
    for path, x in outs.items():
        r = nr.residual_exact(S, x, w)
        if path == "solve":
            r_solve = r
        eta = nr.backward_error(S, x, w, r)
        _seen(path, family, eta / U)
        steps = b.dec["steps"] if path in ("solve", "resid", "full") else 0
        bound = _direct_bound(k, steps)
        assert eta <= bound, (path, family, b.dec, eta / U, bound / U)
    _check_partials(S, outs["solve"], w, r_solve, b.partials, k)
    if hasattr(b, "early"):
        # the fused residual of a reduction forced to stop early is an ESTIMATE of the residual
        # of the returned x: a row next to another workgroup's rows takes their x from its own
        # window (k_solve_pcr), whose copy differs from what that workgroup returns by the same
        # truncation the early stop leaves in x.  Bounded by it: |sqrt(got) - ||r|| | <=
        # 2 || |S| |x - x_exact| ||_2 (x_exact: the full-level solve, exact to ~u)
        x, part = b.early
        r = nr.residual_exact(S, x, w)
        want = math.fsum((r * r).tolist())
        got = math.fsum(part.tolist())
        assert want > 1e-26 * float(w @ w), "the early stop is exact: nothing measured"
        trunc = float(np.linalg.norm(abs(S) @ np.abs(x - outs["solve"])))
        assert abs(math.sqrt(got) - math.sqrt(want)) <= 2 * trunc + 1e-12 * math.sqrt(want), \
            (got, want, trunc)
        print("early stop %s: fused residual off by %.2g of the truncation"
              % (family, abs(math.sqrt(got) - math.sqrt(want)) / trunc))
    return b


def _check_partials(S, x, w, r, part, k):
    """sum(partials) = ||fl(w - S x)||^2 within the gamma bound from the exact residual, or
    both are rounding noise below 1e-28 ||w||^2."""
    got = math.fsum(part.tolist())
    want = math.fsum((r * r).tolist())
    mag = np.abs(w) + abs(S) @ np.abs(x)
    delta = 1.01 * nr.gamma(2 * k + 2) * mag                    # per-row error of fl(w - S x)
    slack = float(np.sum(2 * np.abs(r) * delta + delta * delta)) + \
        float(nr.gamma(len(w) + len(part))) * float(np.sum((np.abs(r) + delta) ** 2))
    noise = 1e-28 * float(w @ w)
    assert abs(got - want) <= slack or (got <= noise and want <= noise), (got, want, slack)


def check_dense(env, A, e, w, family, S=None):
    from ipsolver.dense import DenseNormalSolver
    Ae = nr.pow2_rows(A, e)
    S = nr.gram_pow2(A, e) if S is None else S
    solver = DenseNormalSolver(env.dv.DeviceCSR.from_scipy(Ae))
    x = solver.solve(env.dv.DVec.from_host(w)).to_host()
    eta = nr.backward_error(S, x, w)
    kappa = nr.scaled_cond(S)
    m = A.shape[0]
    _seen("dense/(m k)", family, eta / (U * m * kappa))
    assert eta <= C_DENSE * m * U * kappa, (family, eta / U, m, kappa)
    return x


def check_pcg(env, A, e, w, family, S=None, precond="block"):
    """The CG within its stopping rule on the true residual (C_CG above), no warning."""
    from ipsolver.projector import IterativeNormalSolver as It
    Ae = nr.pow2_rows(A, e)
    S = nr.gram_pow2(A, e) if S is None else S
    solver = It(env.dv.DeviceCSR.from_scipy(Ae), precond=precond)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                      # no "stopped at" warning
        x = solver.solve(env.dv.DVec.from_host(w)).to_host()
    done = float(solver.state[It.PS_DONE].item())
    assert done in (1.0, 2.0), done
    r = nr.residual_exact(S, x, w)
    nw, nres = float(np.linalg.norm(w)), float(np.linalg.norm(r))
    floor = float(np.linalg.norm(abs(S) @ np.abs(x) + np.abs(w)))
    tol = 10 * It.RTOL if done == 1.0 else It.WARN_RELRES
    _seen("pcg-" + precond, family, max(0.0, nres - tol * nw) / (U * floor))
    _seen("pcg-" + precond + ":eta", family, nr.backward_error(S, x, w, r) / U)
    assert nres <= tol * nw + C_CG * U * floor, (family, precond, done, nres / nw, floor / nw)
    return x, solver.stats["iterations"]


# ------------------------------------------------------------------------------ shapes
_ROWS_WG = {}


def rows_per_workgroup(env, k):
    """(rows per workgroup of the single-launch solve, rows per chunk q) for half bandwidth k,
    read from a decoupled factorization (ipx_banded_decoupled_geometry, ipx_banded_chunk_rows)."""
    if k not in _ROWS_WG:
        rng = np.random.default_rng(99)
        A = band_rows(rng, 2600 if k >= 5 else 1200, k, lim=2 ** 4, private=True)
        b = Banded(env, A)
        assert b.geo is not None, ("not decoupled", k, b.dec)
        rows_wg, q = b.geo[0], int(env.lib.ipx_banded_chunk_rows(b.h))
        assert q > k and rows_wg % q == 0 and b.geo[1] == -(-(-(-A.shape[0] // q)) // (rows_wg // q))
        _ROWS_WG[k] = (rows_wg, q)
    return _ROWS_WG[k]


def shapes(env, k):
    """m at the workgroup boundaries of the single-launch solve (j rows_wg + {-1, 0, +1}),
    m = 1 (mod q) (a last chunk of one row) and m below one workgroup; past 2048 rows for
    k >= 5 (shorter bands are one serially swept chunk)."""
    rows_wg, q = rows_per_workgroup(env, k)
    j = 1 if k < 5 else -(-2050 // rows_wg)
    out = [j * rows_wg - 1, j * rows_wg, j * rows_wg + 1, (j + 2) * rows_wg + 1,
           (j + 1) * rows_wg + q + 1]
    if k < 5:
        out.append(rows_wg // 2 + 3)
    assert out[4] % q == 1
    return out


def _rhs(rng, m, spread=0):
    return rng.standard_normal(m) * np.ldexp(1.0, rng.integers(-spread, spread + 1, m))


# ------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7, 8])
def test_random_band_every_path_at_the_workgroup_edges(env, k):
    """(a) Well-conditioned random integer bands, half bandwidth 1..8, at every edge shape
    (diagonally dominant: the single-launch solve at its workgroup boundaries), and at the
    first shape without the dominant column too (separators coupled from k = 3 on): every
    banded form, the dense path (m <= 600) and the CG within their bounds."""
    rng = np.random.default_rng(10 + k)
    for idx, (m, private) in enumerate([(shapes(env, k)[0], False)] +
                                       [(m, True) for m in shapes(env, k)]):
        A = band_rows(rng, m, k, private=private)
        e = np.zeros(m, np.int64)
        w = _rhs(rng, m, 4)
        S = nr.gram_pow2(A, e)
        check_banded(env, A, e, w, "a:k%d" % k, S)
        if idx <= 1:
            if m <= 600:
                check_dense(env, A, e, w, "a:k%d" % k, S)
            check_pcg(env, A, e, w, "a:k%d" % k, S, "block")
            check_pcg(env, A, e, w, "a:k%d" % k, S, "jacobi")


@pytest.mark.parametrize("k", [1, 2, 3, 4, 6, 8])
@pytest.mark.parametrize("grading", ["random", "neighbours"])
def test_graded_rows_every_path(env, k, grading):
    """(b) The same bands with rows scaled by 2^e, e in [-30, 30]: random, and neighbours at
    the two ends of the range.  The scaled backward error obeys the unscaled bound; the
    decisions of the factorization are recorded against the unscaled matrix's."""
    rng = np.random.default_rng(40 + k + (grading == "neighbours"))
    m = shapes(env, k)[3]
    A = band_rows(rng, m, k)
    e = rng.integers(-30, 31, m) if grading == "random" else np.where(np.arange(m) % 2, 30, -30)
    w = _rhs(rng, m, 30)
    S = nr.gram_pow2(A, e)
    plain = Banded(env, A).dec
    family = "b:%s:k%d" % (grading, k)
    try:
        b = check_banded(env, A, e, w, family, S)
    except env.proj.BandedNotDecoupled:
        # the contraction bound of defect correction is not scale invariant: grading may push
        # it past 0.5 (IPX_EUNSUPPORTED; the unscaled band was accepted) -- a decision that
        # moved; the solvers taken instead are checked below
        assert k >= 5 and (plain["decoupled"] or plain["steps"]), plain
        print("graded %s k=%d: decisions unscaled %s -> graded IPX_EUNSUPPORTED"
              % (grading, k, plain))
    else:
        moved = {key: (plain[key], b.dec[key]) for key in plain if plain[key] != b.dec[key]}
        print("graded %s k=%d: decisions unscaled -> graded: %s" % (grading, k, moved or "same"))
    if m <= 800:
        check_dense(env, A, e, w, family, S)
    check_pcg(env, A, e, w, family, S, "block")
    check_pcg(env, A, e, w, family, S, "jacobi")


@pytest.mark.parametrize("k", [1, 3])
def test_graded_rows_at_1e5(env, k):
    """m = 1e5: random grading, one right-hand side."""
    rng = np.random.default_rng(70 + k)
    m = 100000
    A = band_rows(rng, m, k)
    e = rng.integers(-30, 31, m)
    check_banded(env, A, e, _rhs(rng, m, 30), "b:1e5:k%d" % k)


@pytest.mark.parametrize("k,W,eps", [(1, 4096, 1), (1, 2048, 3), (3, 1024, 1), (6, 512, 1),
                                     (8, 512, 2)])
def test_nearly_dependent_neighbours_are_not_ill_conditioned(env, k, W, eps):
    """(c) Integer moving averages plus a small private column: cond(S) ~1e6 at 1500 rows
    and ~5e7 at 20000 (as far as 26-bit entries of S allow), no pivot losing 43 bits --
    ipx_banded_status is IPX_OK, not IPX_EILLCOND -- and every path within its bound."""
    rng = np.random.default_rng(k + W + eps)
    m = 20000 if k <= 3 else 1500
    A = moving_average(m, k, W, eps, rng, noise=3)
    e = np.zeros(m, np.int64)
    S = nr.gram_pow2(A, e)
    w = _rhs(rng, m)
    b = check_banded(env, A, e, w, "c:k%d" % k, S, expect_status=IPX_OK)
    print("moving average k=%d W=%d eps=%d: decisions %s" % (k, W, eps, b.dec))


def test_cyclic_reduction_decision_edges(env):
    """(d) Tridiagonal Toeplitz S (rows W, W on two columns, eps private; coupling ratio
    W^2 / (2 W^2 + eps^2)) tuned so that the reduction decouples at exactly L = 6 (and the
    chunk separators decouple), at exactly L = 7 (coupling at distance 64 just above 2^-56,
    separators 65 apart just below it), and not by level 7 (separators coupled: the chunked
    factorization).  The decisions are asserted so that each case stays at its edge."""
    rng = np.random.default_rng(3)
    m = 3000
    cases = [(8, 7, 6, 1), (36, 22, 7, 1), (36, 12, 0, 0)]
    for W, eps, L, dec in cases:
        A = moving_average(m, 1, W, eps)
        e = np.zeros(m, np.int64)
        w = _rhs(rng, m)
        b = check_banded(env, A, e, w, "d:pcr:L%d" % L)
        assert (b.dec["decoupled"], b.dec["L"]) == (dec, L), (W, eps, b.dec)


def test_graded_separators_are_tested_against_both_diagonals(env):
    """Tridiagonal Toeplitz S whose chunk separators couple at ~2^-80 of the diagonal (the
    reduction decouples at L = 6), rows scaled by 2^e, e random in [-30, 30]: a separator
    coupling is tested against the diagonal entries of both separators it joins
    (k_decoupling_check), so whatever the factorization decides, every path meets the bound."""
    rng = np.random.default_rng(21)
    m = 3000
    A = moving_average(m, 1, 8, 7)
    e = rng.integers(-30, 31, m)
    b = check_banded(env, A, e, _rhs(rng, m, 30), "graded-separators")
    print("graded separators: %s" % b.dec)
    # three separators, the first scaled by 2^30 and the others by 2^-30: the coupling of
    # separators 0 and 1 is 2^-140 of the first one's diagonal entry but 2^-20 of the second's
    _, q = rows_per_workgroup(env, 1)
    m = 3 * q + 10
    A = moving_average(m, 1, 8, 7)
    e = np.zeros(m, np.int64)
    e[q - 1], e[2 * q - 1], e[3 * q - 1] = 30, -30, -30
    b = check_banded(env, A, e, _rhs(rng, m, 30), "graded-separators")
    assert b.dec["decoupled"] == 0, b.dec


def test_graded_ramp_does_not_lower_the_reduction_level(env):
    """Regression: the cyclic reduction's level check compared a coupling with the diagonal
    entry of ONE of its rows.  Rows scaled up along the band (2^(2l - 30) within blocks of 31)
    make every such test lenient by 2^(2 distance): the check stopped at L = 3 with couplings
    of 2^-45 of the smaller diagonal entry left in -- an inexact solve.  Now both rows' entries
    bound it: the level of the unscaled matrix, and the backward error bound."""
    rng = np.random.default_rng(8)
    A, e = ramp_blocks(40)
    m = A.shape[0]
    plain = Banded(env, A).dec
    assert plain["decoupled"] == 1 and plain["L"] == 4, plain
    w = _rhs(rng, m, 30)
    b = check_banded(env, A, e, w, "ramp")
    assert b.dec["L"] >= plain["L"], (plain, b.dec)


def _raw_status(env, A, k):
    """(ipx_banded_status, decisions) of a handle made for A directly: the contraction bound
    can be read also when the status refuses the factorization (BandedNormalSolver raises)."""
    lib, dv, torch = env.lib, env.dv, env.torch
    Ad = dv.DeviceCSR.from_scipy(A)
    p, m = Ad.pattern, A.shape[0]
    band = torch.empty((k + 1) * m, dtype=torch.float64, device="cuda")
    env.hip.call("ipx_aat_band_w", m, k, dv._p(p.indptr), dv._p(p.indices), dv._p(Ad.val), None,
                 None, dv._p(band), dv.stream_ptr())
    h = ctypes.c_void_p(lib.ipx_banded_create(m, k, 64))
    assert h.value
    try:
        env.hip.call("ipx_banded_factor", h, dv._p(band), dv.stream_ptr())
        return int(lib.ipx_banded_status(h, dv.stream_ptr())), _decisions(lib, h)
    finally:
        lib.ipx_banded_destroy(h)


# (k, eps under, its bound, eps over, its bound): moving averages of weight 256 (noise +-8,
# seed k) whose contraction bound crosses 0.5 between the two private-column weights, as
# measured in a sweep of eps (steps of 1 for k = 5, 6; of 8 for k = 7, 8)
CONTRACTION_EDGES = [(5, 54, 0.4755, 53, 0.5004), (6, 61, 0.4931, 60, 0.5123),
                     (7, 88, 0.4021, 80, 0.5078), (8, 96, 0.4817, 88, 0.5814)]


@pytest.mark.parametrize("k,eps_under,eta_under,eps_over,eta_over", CONTRACTION_EDGES)
def test_defect_correction_at_its_contraction_limit(env, k, eps_under, eta_under, eps_over,
                                                    eta_over):
    """(d) Half bandwidths 5..8 past 2048 rows, separators coupled, the private column tuned by
    one unit on either side of the limit: a contraction bound just under 0.5 gives defect
    correction with its largest step counts, within C_ITER; just over it (read from the
    refused handle), IPX_EUNSUPPORTED, and ``projections`` takes the preconditioned CG."""
    from ipsolver.projector import BandedNotDecoupled, IterativeNormalSolver
    m = 20000
    rng = np.random.default_rng(k)
    under = moving_average(m, k, 256, eps_under, rng, noise=8)
    rng = np.random.default_rng(k)
    over = moving_average(m, k, 256, eps_over, rng, noise=8)
    e = np.zeros(m, np.int64)
    rc, dec = _raw_status(env, over, k)
    print("contraction k=%d: eps %d -> %s (rc %d)" % (k, eps_over, dec, rc))
    assert rc == IPX_EUNSUPPORTED and dec["steps"] == 0, (rc, dec)
    assert 0.5 <= dec["eta"] and abs(dec["eta"] - eta_over) <= 1e-3, dec
    w = _rhs(np.random.default_rng(k + 1), m)
    b = check_banded(env, under, e, w, "d:iter:k%d" % k)
    print("contraction k=%d: eps %d -> %s" % (k, eps_under, b.dec))
    assert b.dec["decoupled"] == 0 and b.dec["steps"] >= 40, b.dec
    assert b.dec["eta"] < 0.5 and abs(b.dec["eta"] - eta_under) <= 1e-3, b.dec
    with pytest.raises(BandedNotDecoupled):
        env.proj.BandedNormalSolver(env.dv.DeviceCSR.from_scipy(over))
    Z, _, _ = env.proj.projections(env.dv.DeviceCSR.from_scipy(over))
    assert isinstance(Z.projector.solver, IterativeNormalSolver)
    check_pcg(env, over, e, w, "d:iter-over:k%d" % k, nr.gram_pow2(over, e))


def _box_matrix(rng, m, k):
    """General rows J (a band: half bandwidth k in J J') with an integer slack each, and two
    bound rows -e_j' + s, +e_j' + s per variable (entries +-1, integer slacks >= 1)."""
    J = band_rows(rng, m, k, lim=2 ** 6)
    n = J.shape[1]
    I = sps.eye(n, format="csr")
    s = rng.integers(1, 9, m + 2 * n).astype(np.float64)
    A = sps.bmat([[J, sps.diags(s[:m]), None, None],
                  [-I, None, sps.diags(s[m:m + n]), None],
                  [I, None, None, sps.diags(s[m + n:])]], format="csr")
    A.sort_indices()
    return A, m


@pytest.mark.parametrize("grading", ["none", "random"])
def test_box_schur_with_graded_general_rows(env, grading):
    """The box-Schur elimination with the general rows scaled by 2^e (the bound rows stay in
    box form, so the compact group tables stay in use: args.grp2), within C_BOX (k + 1) u."""
    from ipsolver.boxschur import BoxSchurNormalSolver
    rng = np.random.default_rng(5 + (grading == "random"))
    A, mg = _box_matrix(rng, 1500, 2)
    M = A.shape[0]
    e = np.zeros(M, np.int64)
    if grading == "random":
        e[:mg] = rng.integers(-30, 31, mg)
    Ae = nr.pow2_rows(A, e)
    solver = BoxSchurNormalSolver(env.dv.DeviceCSR.from_scipy(Ae))
    args = solver.c_args()
    assert args is not None and args.grp2
    S = nr.gram_pow2(A, e)
    w = _rhs(rng, M, 20)
    x = solver.solve(env.dv.DVec.from_host(w)).to_host()
    eta = nr.backward_error(S, x, w)
    _seen("boxschur", grading, eta / U)
    assert eta <= C_BOX * (solver.inner.k + 1) * U, eta / U


# ------------------------------------------------------------- power-of-two equivariance
SHIFTS = [-100, -37, 41, 100]


@pytest.mark.parametrize("family,k", [("a", 1), ("a", 3), ("a", 6), ("b", 1), ("b", 4),
                                      ("c", 1)])
def test_uniform_scaling_is_exact(env, family, k):
    """Every row and the right-hand side scaled by 2^s (s in -100, -37, 41, 100): every
    decision of the factorization identical, every output the unscaled one times 2^-s bit for
    bit -- the banded forms, the dense path and the CG (same iteration count).  Everything
    scales exactly, so a difference is an absolute constant in a kernel or the host."""
    rng = np.random.default_rng(500 + k + ord(family))
    if family == "c":
        m = 1200
        A = moving_average(m, k, 2048, 3, rng, noise=3)
    else:
        m = shapes(env, k)[3]
        A = band_rows(rng, m, k)
    e0 = rng.integers(-30, 31, m) if family == "b" else np.zeros(m, np.int64)
    w = _rhs(rng, m, 30 if family == "b" else 0)

    def run(s):
        Ae = nr.pow2_rows(A, e0 + s)
        b = Banded(env, Ae)
        outs = b.run(np.ldexp(w, s))
        from ipsolver.dense import DenseNormalSolver
        from ipsolver.projector import IterativeNormalSolver
        Ad = env.dv.DeviceCSR.from_scipy(Ae)
        ws = env.dv.DVec.from_host(np.ldexp(w, s))
        if m <= 2000:
            outs["dense"] = DenseNormalSolver(Ad).solve(ws).to_host()
        its = {}
        for pre in ("block", "jacobi"):
            it = IterativeNormalSolver(Ad, precond=pre)
            outs["pcg-" + pre] = it.solve(ws).to_host()
            its[pre] = it.stats["iterations"]
        return b.dec, outs, its

    dec0, out0, its0 = run(0)
    for s in SHIFTS:
        dec, outs, its = run(s)
        assert dec == dec0, (s, dec0, dec)
        assert its == its0, (s, its0, its)
        assert outs.keys() == out0.keys()
        for path in out0:
            want = np.ldexp(out0[path], -s)
            bad = np.flatnonzero(outs[path] != want)
            assert len(bad) == 0, (s, path, bad[:5], outs[path][bad[:3]], want[bad[:3]])


@pytest.mark.parametrize("s", [-37, 41])
def test_uniform_scaling_of_the_box_schur_general_rows(env, s):
    """Box-Schur with its general rows scaled by 2^s: the general part of the solution is the
    unscaled one times 2^-s, the bound part unchanged, bit for bit."""
    from ipsolver.boxschur import BoxSchurNormalSolver
    rng = np.random.default_rng(77)
    A, mg = _box_matrix(rng, 1500, 2)
    M = A.shape[0]
    w = _rhs(rng, M)
    outs = []
    for shift in (0, s):
        e = np.zeros(M, np.int64)
        e[:mg] = shift
        solver = BoxSchurNormalSolver(env.dv.DeviceCSR.from_scipy(nr.pow2_rows(A, e)))
        assert solver.c_args().grp2
        outs.append(solver.solve(env.dv.DVec.from_host(np.ldexp(w, e))).to_host())
    want = outs[0].copy()
    want[:mg] = np.ldexp(want[:mg], -s)
    bad = np.flatnonzero(outs[1] != want)
    assert len(bad) == 0, (bad[:5], outs[1][bad[:3]], want[bad[:3]])


# ---------------------------------------------------------- the deferred verdict, L moving
def test_deferred_verdict_when_the_level_moves(env):
    """A tridiagonal pattern factored with a clean blocking verdict at level L1, then refreshed
    through ``BandedNormalSolver(A2, deferred=...)`` (ipx_banded_refactor) with values that need
    L2 > L1: the verdict word is set, the solve made with the stale level is inexact (its
    backward error is far outside the bound: it must be rejected), and after
    ipx_banded_status the repeated solve meets the bound at the new level.  Refreshed again
    with values that need fewer levels than assumed: either verdict, but the solve meets the
    bound."""
    torch, dv, proj, lib = env.torch, env.dv, env.proj, env.lib
    rng = np.random.default_rng(12)
    m = 4000
    e = np.zeros(m, np.int64)
    mats = {eps: moving_average(m, 1, 8, eps, rng, noise=1) for eps in (100, 16, 40)}
    A1 = mats[100]
    pattern_dev = dv.DeviceCSR.from_scipy(A1)

    def same_pattern(A):
        assert np.array_equal(A.indices, A1.indices) and np.array_equal(A.indptr, A1.indptr)
        return dv.DeviceCSR(pattern_dev.pattern, torch.from_numpy(A.data.copy()).cuda())

    def level(A):
        return Banded(env, A).dec["L"]

    L1, L2, L3 = level(mats[100]), level(mats[16]), level(mats[40])
    assert L1 >= 1 and L2 >= L1 + 1 and L3 < L2, (L1, L2, L3)

    class Deferred:
        verdict = torch.zeros(2, dtype=torch.float64, device="cuda")

    full = proj.BandedNormalSolver(same_pattern(A1))
    assert lib.ipx_banded_pcr_level(_h(full)) == L1
    del full                                                  # -> the pattern's handle pool
    w = _rhs(rng, m)
    S2 = nr.gram_pow2(mats[16], e)
    lazy = proj.BandedNormalSolver(same_pattern(mats[16]), deferred=Deferred)
    assert lazy.pending
    stale = lazy.solve(dv.DVec.from_host(w)).to_host()
    verdict = dv.read_doubles(Deferred.verdict, 1)[0]
    eta_stale = nr.backward_error(S2, stale, w)
    assert verdict != 0.0, "the stale level was accepted"
    assert eta_stale > 1e3 * _direct_bound(1, 0), eta_stale / U     # and it had to be rejected
    assert lib.ipx_banded_status(_h(lazy), dv.stream_ptr()) == IPX_OK
    assert lib.ipx_banded_pcr_level(_h(lazy)) == L2
    again = lazy.solve(dv.DVec.from_host(w)).to_host()
    eta = nr.backward_error(S2, again, w)
    _seen("deferred", "L%d->L%d" % (L1, L2), eta / U)
    assert eta <= _direct_bound(1, 0), eta / U
    # fewer levels than the (now clean) assumed L2
    del lazy
    S3 = nr.gram_pow2(mats[40], e)
    lazy = proj.BandedNormalSolver(same_pattern(mats[40]), deferred=Deferred)
    assert lazy.pending
    x = lazy.solve(dv.DVec.from_host(w)).to_host()
    eta = nr.backward_error(S3, x, w)
    _seen("deferred", "L%d->L%d" % (L2, L3), eta / U)
    assert eta <= _direct_bound(1, 0), eta / U
