"""The block-tridiagonal direct (A A')^-1 (csrc/blocktri.hip, ipsolver/blocktri.py): assembly
exact, every solve judged by an exact residual (tests/normal_ref.py) at the edges of the
reduction, pivot signals, power-of-two equivariance, determinism, the projections against the
oracle, and the public call under ``options={"wide_band": "block-tridiagonal"}``.

Bound (u = 2^-53).  Block cyclic reduction is the Cholesky factorization of S in odd-even block
order, and the solve applies the factor's blocks as TRIANGULAR factors (two b x b triangular
solves per pivot block, never an inverse): backward stable, |dS| <= gamma |L||L'| with inner
products of length <= 3 b per level, so in the scaled norms eta <= C_BLOCK L b u, L the number of
levels (ipx_blocktri_levels).  Every test prints eta / (L b u), and beside it the eta of LAPACK's
banded Cholesky (scipy.linalg.solveh_banded) on the same system: the yardstick for what a direct
factorization delivers.
"""
import ctypes

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sps
import scipy.sparse.linalg

import blocktri_cases as bc
import normal_ref as nr

pytestmark = pytest.mark.gpu

U = nr.U
# largest eta / (L b u) measured on an MI355X over every case of this file (printed by the
# tests): 0.0833 -- the single-block case k = 16, m = 16 (L = 1: eta = 1.33 u, LAPACK's banded
# Cholesky 1.94 u on the same system); every case with two or more levels stays below 0.025.
# C_BLOCK = 0.5 is that maximum with a margin of 6 (C_DIRECT, C_DENSE: margins >= 4-5).
MEASURED_RATIO = 0.0833
C_BLOCK = 0.5

SEEN = {}


def _seen(family, ratio, lapack):
    SEEN[family] = max(SEEN.get(family, (0.0, 0.0)), ratio)
    print("eta/(L b u) %-26s %.3g   (eta/u %.3g, LAPACK banded Cholesky eta/u %.3g)"
          % (family, ratio[0], ratio[1], lapack))


@pytest.fixture(scope="module")
def env():
    import torch
    from ipsolver import _hip, blocktri, device as dv, projector

    class NS:
        pass
    ns = NS()
    ns.torch, ns.hip, ns.dv, ns.proj, ns.lib, ns.bt = torch, _hip, dv, projector, _hip.load(), blocktri
    yield ns
    for key in sorted(SEEN):
        print("largest eta/(L b u) %-26s %.3g" % (key, SEEN[key][0]))


def _levels(env, m, b):
    geo = (ctypes.c_int32 * 2)()
    launched = env.lib.ipx_blocktri_levels(m, b, geo)
    assert launched >= 0
    return int(geo[0]), int(geo[1]), int(launched)


def _lapack_eta(S, w):
    """eta of scipy.linalg.solveh_banded (LAPACK dpbsv) on the same system."""
    S = sps.csr_matrix(S)
    k = bc.half_bandwidth(S)
    dense = S.toarray()
    m = dense.shape[0]
    ab = np.zeros((k + 1, m))
    for d in range(k + 1):
        ab[d, :m - d] = np.diagonal(dense, -d)
    x = scipy.linalg.solveh_banded(ab, w, lower=True)
    return nr.backward_error(S, x, w)


def check_solve(env, A, e, w, family, expect_b=None, kappa_family=None):
    Ae = nr.pow2_rows(A, e)
    S = nr.gram_pow2(A, e)
    m = A.shape[0]
    solver = env.bt.BlockTridiagonalNormalSolver(env.dv.DeviceCSR.from_scipy(Ae))
    assert solver.flag_bits == 0 and not solver.ill_conditioned, solver.flag_bits
    if expect_b is not None:
        assert solver.b == expect_b, (solver.k, solver.b)
    L, tail, launched = _levels(env, m, solver.b)
    assert solver.stats["levels"] == L
    wd = env.dv.DVec.from_host(w)
    x = solver.solve(wd).to_host()
    assert x.shape == (m,) and np.all(np.isfinite(x))
    eta = nr.backward_error(S, x, w)
    lap = _lapack_eta(S, w)
    _seen(family, (eta / (L * solver.b * U), eta / U), lap / U)
    assert eta <= C_BLOCK * L * solver.b * U, (family, m, solver.b, L, eta / U)
    return solver, x, eta, lap, L


# ------------------------------------------------------------------------------ 1. assembly
@pytest.mark.parametrize("k,m", [(9, 47), (16, 48), (17, 65), (33, 129)])
@pytest.mark.parametrize("form", ["canonical", "split-duplicates"])
def test_assembly_is_exact(env, k, m, form):
    """D, E of an integer A equal the int64 product block by block, with and without a row
    permutation; padded rows: unit diagonal, zeros elsewhere; nothing past N blocks written.
    Repeated entries ("split-duplicates") are summed by ``DeviceCSR.from_scipy``, as for every
    assembly here: the kernel's contract (include/ipx.h) is sorted rows with every column once,
    and the second form checks that the summed matrix reaches it with the same values."""
    torch, dv = env.torch, env.dv
    assert env.lib.ipx_blocktri_kmax() == env.bt.BLOCK_SIZES[-1] == 64
    rng = np.random.default_rng(1000 * k + m)
    A = bc.band_rows(rng, m, k, lim=bc.lim_for(k))
    b = bc.BLOCK_OF_K[k]
    N = -(-m // b)
    Ain = nr.split_duplicates(A) if form == "split-duplicates" else A
    Ad = dv.DeviceCSR.from_scipy(Ain)
    p = Ad.pattern
    S = nr.aat_int(A)
    # a permutation that keeps the half bandwidth: the rows reversed
    for perm in (None, np.arange(m - 1, -1, -1).astype(np.int32)):
        Sp = S if perm is None else S[perm][:, perm]
        want = np.zeros((N * b, N * b), dtype=np.int64)
        want[:m, :m] = Sp
        want[np.arange(m, N * b), np.arange(m, N * b)] = 1
        sentinel = -7.25
        D = torch.full(((N + 1) * b * b,), sentinel, dtype=torch.float64, device="cuda")
        E = torch.full(((N + 1) * b * b,), sentinel, dtype=torch.float64, device="cuda")
        permd = None if perm is None else torch.from_numpy(perm).cuda()
        env.hip.call("ipx_aat_blocktri", m, b, k, dv._p(p.indptr), dv._p(p.indices), dv._p(Ad.val),
                     dv._p(permd), dv._p(D), dv._p(E), dv.stream_ptr())
        Dh = D.cpu().numpy().reshape(N + 1, b, b)
        Eh = E.cpu().numpy().reshape(N + 1, b, b)
        assert np.all(Dh[N] == sentinel) and np.all(Eh[N] == sentinel)
        assert np.all(Eh[0] == 0)
        for I in range(N):
            assert np.array_equal(Dh[I], want[I * b:(I + 1) * b, I * b:(I + 1) * b]), (perm is None, I)
            if I:
                assert np.array_equal(Eh[I], want[I * b:(I + 1) * b, (I - 1) * b:I * b]), I
        # nothing of S lies outside the two block diagonals
        mask = np.abs(np.arange(N * b)[:, None] // b - np.arange(N * b)[None, :] // b) > 1
        assert not want[mask].any()


# ------------------------------------------------- 2. solves at the edges of the reduction
@pytest.mark.parametrize("k", bc.KS)
def test_solve_by_exact_residual_at_the_edges_of_the_reduction(env, k):
    """m = N b + {-1, 0, 1} for N = 1, 2, 3, 4, 5, 8, 9 (a single block, the first level, odd and
    even counts at the first three levels), N = 2 tail + 1 (two levels as launches of their own
    before the one-workgroup tail), and graded rows (2^e, e in [-30, 30]), plain and
    diagonally dominant: eta <= C_BLOCK L b u."""
    b = bc.BLOCK_OF_K[k]
    for name, m, private, graded in bc.edge_cases(k):
        A, e, w = bc.build(k, name, m, private, graded)
        L, tail, launched = _levels(env, m, b)
        assert tail == bc.TAIL_ROWS[b]
        if name == "launched":
            assert launched == 2, (m, b, launched)
        elif m <= tail * b:
            assert launched == 0
        solver, x, eta, lap, L = check_solve(env, A, e, w, "k%d:%s" % (k, name), b)
        if private:
            # the yardstick of the issue: on the diagonally dominant family the device stays
            # within 16 L of LAPACK's banded Cholesky
            assert eta <= 16 * L * max(lap, U), (k, name, eta / U, lap / U)


# ----------------------------------------------------------------- 3. nearly dependent rows
def test_nearly_dependent_rows_are_not_ill_conditioned(env):
    """moving_average(1500, 11, 512, 1): kappa of the scaled S = 9.0e5 (computed on the host), no
    pivot loses 43 bits: clean status, and the solve within the same bound."""
    A = bc.moving_average(1500, 11, 512, 1)
    m = A.shape[0]
    rng = np.random.default_rng(11)
    w = rng.standard_normal(m)
    kappa = nr.scaled_cond(nr.gram_pow2(A))
    print("moving average: kappa of the scaled S %.3g" % kappa)
    assert kappa > 1e5
    solver, *_ = check_solve(env, A, np.zeros(m, np.int64), w, "moving-average:k11", 16)
    assert solver.k == 11 and not solver.ill_conditioned


# ------------------------------------------------------------------------- 4. pivot signals
def test_zero_row_is_refused(env):
    rng = np.random.default_rng(5)
    A = bc.band_rows(rng, 70, 9, lim=2 ** 8).tolil()
    A.rows[20], A.data[20] = [], []
    with pytest.raises(np.linalg.LinAlgError, match="not positive definite"):
        env.bt.BlockTridiagonalNormalSolver(env.dv.DeviceCSR.from_scipy(A.tocsr()))


def test_identical_rows_are_refused(env):
    """Rows 16 and 17 identical, sixteen entries +-4: they open block row 1 (b = 16), an odd row
    of the first level, which is factored from the ORIGINAL integer entries.  Pivot 16 is
    S = 256, its square root 16 and the quotient 256 / 16 are exact, so pivot 17 is
    256 - 16 * 16 = 0 exactly: not positive, LinAlgError (not merely ill-conditioned).  The same
    through ``projections``: the SVD exit, with the reference's warning."""
    A = bc.identical_rows(np.random.default_rng(4))
    with pytest.raises(np.linalg.LinAlgError, match="not positive definite"):
        env.bt.BlockTridiagonalNormalSolver(env.dv.DeviceCSR.from_scipy(A))
    with env.proj.wide_band("block-tridiagonal"):
        with pytest.warns(UserWarning, match="Singular Jacobian"):
            Z, _, _ = env.proj.projections(env.dv.DeviceCSR.from_scipy(A))
    assert isinstance(Z.projector, env.proj.SVDProjector)


# ------------------------------------------------------------ 5. uniform scaling is exact
@pytest.mark.parametrize("k,N", [(9, 5), (33, 3), (16, 65)])
def test_uniform_scaling_is_exact(env, k, N):
    """Every row and w scaled by 2^s: S scales by 4^s, every square root and quotient scales
    exactly -- the output is the unscaled one times 2^-s bit for bit, the flags the same."""
    b = bc.BLOCK_OF_K[k]
    m = N * b + 1
    A, e0, w = bc.build(k, "scaling", m, False, True)

    def run(s):
        solver = env.bt.BlockTridiagonalNormalSolver(
            env.dv.DeviceCSR.from_scipy(nr.pow2_rows(A, e0 + s)))
        return solver.flag_bits, solver.solve(env.dv.DVec.from_host(np.ldexp(w, s))).to_host()

    bits0, x0 = run(0)
    assert bits0 == 0
    for s in (-100, -37, 41, 100):
        bits, x = run(s)
        assert bits == bits0
        want = np.ldexp(x0, -s)
        bad = np.flatnonzero(x != want)
        assert len(bad) == 0, (s, bad[:5], x[bad[:3]], want[bad[:3]])


# ------------------------------------------------------------------------- 6. determinism
@pytest.mark.parametrize("k,N", [(17, 9), (9, 65)])
def test_factorization_and_solve_are_deterministic(env, k, N):
    b = bc.BLOCK_OF_K[k]
    m = N * b - 1
    A, e, w = bc.build(k, "determinism", m, False, True)
    Ad = env.dv.DeviceCSR.from_scipy(nr.pow2_rows(A, e))
    wd = env.dv.DVec.from_host(w)
    one, two = (env.bt.BlockTridiagonalNormalSolver(Ad) for _ in range(2))
    nb = -(-m // b)
    # D and E (the factor's L and U blocks; V of a block row without a right neighbour is
    # never written, so V is compared through the solves)
    assert np.array_equal(one.ws[:2 * nb * b * b].cpu().numpy(), two.ws[:2 * nb * b * b].cpu().numpy())
    xs = [one.solve(wd).to_host(), one.solve(wd).to_host(), two.solve(wd).to_host()]
    assert np.array_equal(xs[0], xs[1]) and np.array_equal(xs[0], xs[2])


# -------------------------------------------------------- 7. projections against the oracle
def test_projections_under_the_policy_against_the_oracle(env, monkeypatch):
    import oracle
    from ipsolver.dense import DenseNormalSolver
    proj, dv = env.proj, env.dv
    rng = np.random.default_rng(7)
    A = bc.ocp_rows(12, 4, 40, rng)
    m, n = A.shape
    Zo, LSo, Yo = oracle.projections(A)
    x, b = rng.standard_normal(n), rng.standard_normal(m)
    Ad = dv.DeviceCSR.from_scipy(A)
    with proj.wide_band("block-tridiagonal"):
        Z, LS, Y = proj.projections(Ad)
        solver = Z.projector.solver
        assert isinstance(solver, proj.BlockTridiagonalNormalSolver)
        assert (solver.k, solver.b) == (23, 32)
        assert proj.last_normal_solver() == "BlockTridiagonalNormalSolver"
        z = Z.dot(x).to_host()
        rel = lambda a, want: np.max(np.abs(a - want)) / max(1.0, np.max(np.abs(want)))
        assert rel(z, Zo.dot(x)) <= 1e-10
        assert rel(LS.dot(x).to_host(), LSo.dot(x)) <= 1e-10
        assert rel(Y.dot(b).to_host(), Yo.dot(b)) <= 1e-10
        assert np.linalg.norm(A @ z) <= 1e-12 * scipy.sparse.linalg.norm(A) * np.linalg.norm(z)
        # the fused CG loop does not take this solver: host-driven loop
        from ipsolver import cg_fused
        assert cg_fused._solver_kind(solver) is None
    # outside the context: a new factorization (the policy is part of the cache key), today's
    assert proj.wide_band_policy() == "iterative"
    Z2, _, _ = proj.projections(Ad)
    assert isinstance(Z2.projector.solver, DenseNormalSolver)
    monkeypatch.setattr(DenseNormalSolver, "MAX_ROWS_FROM_SPARSE", 100)
    Z3, _, _ = proj.projections(dv.DeviceCSR.from_scipy(A))
    assert isinstance(Z3.projector.solver, proj.IterativeNormalSolver)
    # half bandwidth 70 under the policy: past ipx_blocktri_kmax, today's path
    A70 = bc.band_rows(rng, 300, 70, lim=2 ** 4)
    with proj.wide_band("block-tridiagonal"):
        Z4, _, _ = proj.projections(dv.DeviceCSR.from_scipy(A70))
        assert isinstance(Z4.projector.solver, proj.IterativeNormalSolver)
        with pytest.raises(NotImplementedError, match="half bandwidth 70"):
            proj.BlockTridiagonalNormalSolver(dv.DeviceCSR.from_scipy(A70))
    monkeypatch.undo()
    with proj.wide_band("block-tridiagonal"):
        Z5, _, _ = proj.projections(dv.DeviceCSR.from_scipy(A70))
    assert isinstance(Z5.projector.solver, DenseNormalSolver)


def test_a_reused_factorization_is_still_named(env):
    """``projections`` on unchanged values returns its cached operators; the solver behind
    them is still what ``last_normal_solver`` (the result's ``normal_solver``) names."""
    proj = env.proj
    Ad = env.dv.DeviceCSR.from_scipy(bc.ocp_rows(6, 2, 30, np.random.default_rng(3)))
    with proj.wide_band("block-tridiagonal"):
        first = proj.projections(Ad)
        proj._last_solver[0] = None                       # (what the driver does per call)
        again = proj.projections(Ad)
        assert again is first
        assert proj.last_normal_solver() == "BlockTridiagonalNormalSolver"


# --------------------------------------------------------------- 8. through the public call
@pytest.mark.parametrize("box", [True, False])
def test_public_call_with_the_wide_band_option(env, box):
    """A staged problem (d = 6, c = 2, 30 stages: J J' of half bandwidth 11), quadratic
    objective, sparse NonlinearConstraint ('equals', 0), with and without a box on every
    variable: the same solution under both policies, ``normal_solver`` naming the solver."""
    import ipsolver
    J, rhs, target = bc.staged_problem()
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

    wide = solve({"wide_band": "block-tridiagonal"})
    default = solve({})
    assert env.proj.wide_band_policy() == "iterative"
    assert wide.status in (1, 2) and default.status in (1, 2), (wide.status, default.status)
    assert np.max(np.abs(wide.x - default.x)) <= 1e-6
    assert np.max(np.abs(J @ wide.x - rhs)) <= 1e-7
    print("normal_solver: %s (wide), %s (default); niter %d / %d"
          % (wide.normal_solver, default.normal_solver, wide.niter, default.niter))
    if box:
        assert wide.normal_solver == "BoxSchurNormalSolver/BlockTridiagonalNormalSolver"
    else:
        assert wide.normal_solver == "BlockTridiagonalNormalSolver"
    assert isinstance(default.normal_solver, str) and "BlockTridiagonal" not in default.normal_solver
