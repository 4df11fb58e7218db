"""The bordered direct (A A')^-1 (csrc/bordered.hip, ipsolver/bordered.py): every solve judged by
an exact residual (tests/normal_ref.py) at the edges of the partial counts, dominant columns
under refinement, the guards, power-of-two equivariance, determinism, the projections against the
oracle, and the public call under ``options={"border_columns": ...}``.

Bound (u = 2^-53).  Woodbury on a backward-stable inner solve: eta <= c kappa_B kappa_2(K) u plus
the inner solver's own error, and kappa_2(K) <= trace(K) since K >= I.  c comes from the host twin
(the same formula in numpy with LAPACK's Cholesky; C_TWIN, tests/test_bordered_host.py) with a
margin of 8 -- the device's inner solve is cyclic reduction, not LAPACK's Cholesky, and its sums
run in another order -- and the inner term is the inner solver's asserted bound
(tests/test_gpu_normal_solve.py, tests/test_gpu_blocktri.py):

    eta <= (8 C_TWIN kappa_B trace(K) + C_inner) u.

Every case prints eta / u beside the twin's and LAPACK's dense Cholesky of the full S.
Measured on an MI355X so far: the first ten solve cases only (k = 1; m = 1, 2, 255), eta = 0.016
... 11.7 u, largest eta / bound 0.036 (m = 1, p = 31, graded: 11.7 u, twin 0.98 u, LAPACK 0.29 u);
the remaining cases have not run on a GPU yet.
"""
import ctypes
import warnings

import numpy as np
import pytest
import scipy.sparse as sps
import scipy.sparse.linalg

import blocktri_cases as bc
import bordered_cases as bd
import normal_ref as nr

pytestmark = pytest.mark.gpu

U = nr.U
C_DIRECT, C_ITER = 4.0, 8.0          # tests/test_gpu_normal_solve.py: eta <= C (k + 1) u
C_BLOCK = 0.5                        # tests/test_gpu_blocktri.py: eta <= C_BLOCK L b u
# largest eta / bound measured on an MI355X (printed at the end of the module): see the header
MEASURED_RATIO = 0.036

SEEN = {}


@pytest.fixture(scope="module")
def env():
    import torch
    from ipsolver import _hip, blocktri, bordered, device as dv, projector

    class NS:
        pass
    ns = NS()
    ns.torch, ns.hip, ns.dv, ns.proj, ns.lib = torch, _hip, dv, projector, _hip.load()
    ns.bt, ns.bd = blocktri, bordered
    assert ns.lib.ipx_border_rows_per_group() == bd.ROWS_PER_GROUP
    assert ns.lib.ipx_border_pmax() == bd.P_MAX
    yield ns
    for key in sorted(SEEN):
        print("largest eta/bound %-12s %.3g  (eta/u %.3g)" % ((key,) + SEEN[key]))


def _inner_bound(env, inner):
    """The inner solver's own asserted bound, in units of u."""
    if isinstance(inner, env.proj.BandedNormalSolver):
        steps = env.lib.ipx_banded_refine_steps(ctypes.c_void_p(inner.handle), None)
        return (C_ITER if steps else C_DIRECT) * (inner.k + 1)
    assert isinstance(inner, env.bt.BlockTridiagonalNormalSolver)
    return C_BLOCK * inner.stats["levels"] * inner.b


def _solver(env, A, cols, e):
    Ad = env.dv.DeviceCSR.from_scipy(nr.pow2_rows(A, e))
    split = env.bd.split_columns(Ad.pattern, cols)
    assert split is not None and split.p == len(cols)
    return env.bd.BorderedNormalSolver(Ad, split), Ad


def check_solve(env, A, cols, e, w, family, dominant=False):
    m, p = A.shape[0], len(cols)
    S = nr.gram_pow2(A, e)
    B_int, _ = bd.split(A, cols)
    Be, Ce = bd.split(nr.pow2_rows(A, e), cols)
    solver, _ = _solver(env, A, cols, e)
    k_B = bc.half_bandwidth(nr.gram_pow2(B_int))
    want_inner = env.proj.BandedNormalSolver if k_B <= env.lib.ipx_banded_kmax() \
        else env.bt.BlockTridiagonalNormalSolver
    assert type(solver.inner) is want_inner, (k_B, type(solver.inner))
    assert solver.flag_bits == 0 and not solver.ill_conditioned and solver.perm is None
    # C as scattered, K against the twin's
    assert np.array_equal(solver.C.cpu().numpy().reshape(p, m).T, Ce)
    v_twin, K_twin = bd.twin(Be, Ce, w)
    kappa_B = nr.scaled_cond(nr.gram_pow2(B_int, e))
    K_dev = solver.K.cpu().numpy().reshape(p, p)
    low = np.tril_indices(p)
    assert np.max(np.abs(K_dev[low] - K_twin[low])) <= 1e-9 * np.max(np.abs(K_twin))
    trK = float(np.trace(K_twin))
    assert abs(solver.growth - trK) <= 1e-9 * trK
    refined = trK > env.bd.GROWTH_REFINE              # (some p = 31, 32 cases of the band's
    assert solver.refine == refined                   # magnitude pass 2^10 too: refined as well)
    assert refined or not dominant
    x = solver.solve(env.dv.DVec.from_host(w)).to_host()
    assert x.shape == (m,) and np.all(np.isfinite(x))
    assert solver.stats["refinements"] == (1 if refined else 0)
    eta = nr.backward_error(S, x, w)
    eta_twin = nr.backward_error(S, v_twin, w)
    eta_lap = nr.backward_error(S, bd.lapack_dense(S, w), w)
    bound = 8 * bd.C_TWIN * kappa_B * (1.0 if dominant else trK) + _inner_bound(env, solver.inner)
    print("eta/u %-34s %.3g  (twin %.3g, LAPACK dense Cholesky %.3g; bound %.3g: kappa_B %.3g, "
          "trace(K) %.3g%s)" % (family, eta / U, eta_twin / U, eta_lap / U, bound, kappa_B, trK,
                               ", refined" if refined else ""))
    key = family.split(":")[0]
    SEEN[key] = max(SEEN.get(key, (0.0, 0.0)), (eta / (bound * U), eta / U))
    assert eta <= bound * U, (family, eta / U, bound)
    return solver


# ------------------------------------------------- 1. solves at the edges of the partial counts
@pytest.mark.parametrize("k", bd.SOLVE_K)
def test_solve_by_exact_residual(env, k):
    """m in {1, 2, R - 1, R, R + 1, 2 R + 1} (R = ipx_border_rows_per_group(): one, two, three
    partial blocks), p in {1, 2, 31, 32}, fill 1.0 / 0.3, graded (2^e, e in [-30, 30]) and plain
    rows; inner banded (k = 1, 4) and block tridiagonal (k = 9, 17, from m > k on)."""
    R = bd.ROWS_PER_GROUP
    assert [env.lib.ipx_border_groups(m) for m in (1, R, R + 1, 2 * R, 2 * R + 1)] == [1, 1, 2, 2, 3]
    assert env.lib.ipx_border_groups(10 ** 6) == 512
    with env.proj.wide_band("block-tridiagonal" if k > 8 else "iterative"):
        for m, p, fill, graded in bd.solve_cases(k):
            A, cols, e, w = bd.build(k, m, p, fill, graded)
            check_solve(env, A, cols, e, w,
                        "k%d:m%d p%d fill%.1f%s" % (k, m, p, fill, " graded" if graded else ""))


# ---------------------------------------------------------------------- 2. dominant columns
def test_dominant_columns_are_refined(env):
    """|C| up to 64 x the band, p = 32: trace(K) = 3.3e6 > GROWTH_REFINE, one refinement step per
    solve; eta within the bound with trace(K) replaced by 1."""
    A, cols, e, w = bd.dominant_case()
    with env.proj.wide_band("block-tridiagonal"):
        solver = check_solve(env, A, cols, e, w, "dominant:k9", dominant=True)
    assert solver.growth > env.bd.GROWTH_REFINE
    assert solver.stats == {"solves": 1, "refinements": 1, "inner_solves": 32 + 2}


# ------------------------------------------------------------------------------- 3. guards
@pytest.mark.parametrize("case", ["growth", "identical-rows", "border-only-row"])
def test_guards_fall_back_to_todays_solver(env, case):
    proj, dv = env.proj, env.dv
    A, cols = {"growth": bd.huge_growth_case, "identical-rows": bd.identical_rows_case,
               "border-only-row": bd.border_only_row_case}[case]()
    Ad = dv.DeviceCSR.from_scipy(A)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with proj.wide_band("block-tridiagonal"):
            today = proj.projections(dv.DeviceCSR.from_scipy(A))
            name_today = proj.last_normal_solver()
            split = env.bd.split_columns(Ad.pattern, cols)
            if case == "border-only-row":
                assert split is None
            else:
                assert proj.border_split(Ad.pattern, proj.border_reach(), 4) is not None
                with pytest.raises(env.bd.BorderedRefused,
                                   match="trace" if case == "growth" else "B B."):
                    env.bd.BorderedNormalSolver(Ad, split)
            with proj.border_columns(4):
                Z, LS, Y = proj.projections(Ad)
                assert proj.last_normal_solver() == name_today
                assert "Bordered" not in name_today
    assert type(Z.projector) is type(today[0].projector)
    x = np.random.default_rng(1).standard_normal(A.shape[1])
    z, z_today = Z.dot(x).to_host(), today[0].dot(x).to_host()
    assert np.all(np.isfinite(z))
    assert np.max(np.abs(z - z_today)) <= 1e-8 * np.max(np.abs(x))       # the same solver


# ------------------------------------------------------------ 4. uniform scaling is exact
def test_uniform_scaling_is_exact(env):
    """Rows scaled by 2^s (block-tridiagonal inner, exactly equivariant by its own test): K does
    not change, Y scales by 2^-s and, for the same w, v by 4^-s -- bit for bit."""
    k, m, p = 9, bd.ROWS_PER_GROUP + 1, 3
    A, cols, e0, w = bd.build(k, m, p, 0.3, True)

    def run(s):
        solver, _ = _solver(env, A, cols, e0 + s)
        assert isinstance(solver.inner, env.bt.BlockTridiagonalNormalSolver)
        v = solver.solve(env.dv.DVec.from_host(w)).to_host()
        return solver.K.cpu().numpy(), solver.Y.cpu().numpy(), v, solver.growth

    K0, Y0, v0, g0 = run(0)
    for s in (-37, 41):
        K, Y, v, g = run(s)
        assert np.array_equal(K, K0) and g == g0
        assert np.array_equal(np.ldexp(Y, s), Y0)
        bad = np.flatnonzero(np.ldexp(v, 2 * s) != v0)
        assert len(bad) == 0, (s, bad[:5])


# ------------------------------------------------------------------------- 5. determinism
def test_factorization_and_solve_are_deterministic(env):
    k, m, p = 9, 2 * bd.ROWS_PER_GROUP + 1, 31
    A, cols, e, w = bd.build(k, m, p, 1.0, True)
    (one, _), (two, _) = (_solver(env, A, cols, e) for _ in range(2))
    n = 2 * m * p + 2 * p * p + 2                       # C, Y, K, L, info
    assert np.array_equal(one.ws[:n].cpu().numpy(), two.ws[:n].cpu().numpy())
    wd = env.dv.DVec.from_host(w)
    xs = [one.solve(wd).to_host(), one.solve(wd).to_host(), two.solve(wd).to_host()]
    assert np.array_equal(xs[0], xs[1]) and np.array_equal(xs[0], xs[2])


# -------------------------------------------------------- 6. projections against the oracle
def test_projections_under_both_options_against_the_oracle(env):
    import oracle
    from ipsolver import cg_fused
    proj, dv = env.proj, env.dv
    rng = np.random.default_rng(7)
    A, cols = bd.bordered(rng, bc.ocp_rows(12, 4, 40, rng), 3, 1.0, 2 ** 6)
    m, n = A.shape
    Zo, LSo, Yo = oracle.projections(A)
    x, b = rng.standard_normal(n), rng.standard_normal(m)
    Ad = dv.DeviceCSR.from_scipy(A)
    rel = lambda a, want: np.max(np.abs(a - want)) / max(1.0, np.max(np.abs(want)))
    with proj.wide_band("block-tridiagonal"), proj.border_columns(4):
        Z, LS, Y = proj.projections(Ad)
        solver = Z.projector.solver
        assert isinstance(solver, proj.BorderedNormalSolver) and solver.p == 3
        assert proj.last_normal_solver() == "BorderedNormalSolver/BlockTridiagonalNormalSolver"
        assert (solver.inner.k, solver.inner.b) == (23, 32)
        z = Z.dot(x).to_host()
        assert rel(z, Zo.dot(x)) <= 1e-10
        assert rel(LS.dot(x).to_host(), LSo.dot(x)) <= 1e-10
        assert rel(Y.dot(b).to_host(), Yo.dot(b)) <= 1e-10
        assert np.linalg.norm(A @ z) <= 1e-12 * scipy.sparse.linalg.norm(A) * np.linalg.norm(z)
        assert cg_fused._solver_kind(solver) is None          # the host-driven loop
        # a reused factorization is still named
        proj._last_solver[0] = None
        again = proj.projections(Ad)
        assert again[0] is Z
        assert proj.last_normal_solver() == "BorderedNormalSolver/BlockTridiagonalNormalSolver"
    # outside the context: a new factorization (the limit is part of the cache key), today's
    assert proj.border_columns_limit() == 0 and proj.wide_band_policy() == "iterative"
    Z2, _, _ = proj.projections(Ad)
    assert Z2 is not Z and "Bordered" not in proj.last_normal_solver()
    with proj.wide_band("block-tridiagonal"):
        Z3, _, _ = proj.projections(Ad)
        assert Z3 is not Z and "Bordered" not in proj.last_normal_solver()


def test_banded_inner_under_the_default_policy(env):
    """A tridiagonal A A' plus one dense column, the default wide-band policy: the bordered
    solver on the banded one, the operators against the oracle."""
    import oracle
    proj, dv = env.proj, env.dv
    rng = np.random.default_rng(8)
    A, cols = bd.bordered(rng, bc.band_rows(rng, 300, 1, lim=2 ** 4), 1, 0.3, 2 ** 4, where="first")
    Zo, LSo, Yo = oracle.projections(A)
    x, b = rng.standard_normal(A.shape[1]), rng.standard_normal(A.shape[0])
    with proj.border_columns(1):
        Z, LS, Y = proj.projections(dv.DeviceCSR.from_scipy(A))
        assert proj.last_normal_solver() == "BorderedNormalSolver/BandedNormalSolver"
    rel = lambda a, want: np.max(np.abs(a - want)) / max(1.0, np.max(np.abs(want)))
    assert rel(Z.dot(x).to_host(), Zo.dot(x)) <= 1e-10
    assert rel(LS.dot(x).to_host(), LSo.dot(x)) <= 1e-10
    assert rel(Y.dot(b).to_host(), Yo.dot(b)) <= 1e-10


# --------------------------------------------------------------- 7. through the public call
@pytest.mark.parametrize("box", [True, False])
def test_public_call_with_the_border_columns_option(env, box):
    """The staged problem of the block-tridiagonal test (d = 6, c = 2, 30 stages) with two
    global parameter columns in J, with and without a box on every variable: the same solution
    with and without the options, ``normal_solver`` naming the bordered solver."""
    import ipsolver
    J, rhs, target = bd.staged_problem_with_parameters()
    n = J.shape[1]

    def solve(options):
        cons = [ipsolver.NonlinearConstraint(lambda x: J @ x - rhs, ("equals", 0), lambda x: J,
                                             lambda x, v: sps.csr_matrix((n, n)))]
        if box:
            cons.append(ipsolver.BoxConstraint(("interval", -2.0, 2.0)))
        return ipsolver.minimize_constrained(
            lambda x: 0.5 * float((x - target) @ (x - target)), np.zeros(n),
            lambda x: x - target, lambda x: sps.identity(n, format="csr"), cons,
            options=options)

    bordered = solve({"wide_band": "block-tridiagonal", "border_columns": 4})
    default = solve({})
    assert env.proj.border_columns_limit() == 0 and env.proj.wide_band_policy() == "iterative"
    assert bordered.status in (1, 2) and default.status in (1, 2), (bordered.status, default.status)
    assert np.max(np.abs(bordered.x - default.x)) <= 1e-6
    assert np.max(np.abs(J @ bordered.x - rhs)) <= 1e-7
    print("normal_solver: %s (bordered), %s (default); niter %d / %d"
          % (bordered.normal_solver, default.normal_solver, bordered.niter, default.niter))
    name = "BorderedNormalSolver/BlockTridiagonalNormalSolver"
    assert bordered.normal_solver == ("BoxSchurNormalSolver/" + name if box else name)
    assert isinstance(default.normal_solver, str) and "Bordered" not in default.normal_solver
    with pytest.raises(ValueError, match="border_columns"):
        solve({"border_columns": 33})
