"""The linked direct (A A')^-1 (csrc/linked.hip, ipsolver/linked.py): the product P A D' bit for
bit against its definition, every solve judged by an exact residual (tests/normal_ref.py) at the
edges of the partial counts, nearly dependent link rows, the guards, power-of-two equivariance,
determinism, the composition with border columns, the projections against the oracle, and the
public call under ``options={"link_rows": ...}``.

Bound (u = 2^-53).  A block Cholesky of the SPD matrix S on a backward-stable inner solve:
eta <= c kappa_B u plus the inner solver's own error, with no term for the cancellation in K.
c comes from the host twin (the same formula in numpy with LAPACK's Cholesky; C_TWIN_LINK,
tests/test_link_rows_host.py) with a margin of 8 -- the device's inner solve is cyclic reduction,
not LAPACK's Cholesky, and its sums run in another order -- and the inner term is the inner
solver's asserted bound (tests/test_gpu_normal_solve.py, tests/test_gpu_blocktri.py):

    eta <= (8 C_TWIN_LINK kappa_B + C_inner) u.

Every case prints eta / u beside the twin's and LAPACK's dense Cholesky of the full S.
Measured on an MI355X over the 96 solve cases: eta = 0.064 ... 0.762 u against bounds of
14 ... 238 u, largest eta / bound 0.054 (k = 17, m_B = 1, q = 31: 0.762 u, twin 0.273 u, LAPACK
0.682 u); the nearly dependent case 0.15 u (twin 0.21 u, LAPACK 0.47 u).
"""
import ctypes
import warnings

import numpy as np
import pytest
import scipy.sparse as sps
import scipy.sparse.linalg

import blocktri_cases as bc
import bordered_cases as bd
import link_cases as lc
import normal_ref as nr

pytestmark = pytest.mark.gpu

U = nr.U
C_DIRECT, C_ITER = 4.0, 8.0          # tests/test_gpu_normal_solve.py: eta <= C (k + 1) u
C_BLOCK = 0.5                        # tests/test_gpu_blocktri.py: eta <= C_BLOCK L b u

SEEN = {}


@pytest.fixture(scope="module")
def env():
    import torch
    from ipsolver import _hip, blocktri, bordered, linked, device as dv, projector

    class NS:
        pass
    ns = NS()
    ns.torch, ns.hip, ns.dv, ns.proj, ns.lib = torch, _hip, dv, projector, _hip.load()
    ns.bt, ns.bd, ns.lk = blocktri, bordered, linked
    assert ns.lib.ipx_border_rows_per_group() == lc.ROWS_PER_GROUP
    assert ns.lib.ipx_border_pmax() == lc.Q_MAX
    yield ns
    for key in sorted(SEEN):
        print("largest eta/bound %-12s %.3g  (eta/u %.3g)" % ((key,) + SEEN[key]))


def _dev(env, a, dtype):
    return env.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(env.dv.ctx().device)


# ------------------------------------------------------------------ 1. the product, bit for bit
def _product_definition(A, Dt, dst_row):
    """G[dst_row[r], :] = sum over the entries of row r, in storage order, of val * Dt[col, :]:
    one multiply and one add per entry (numpy rounds each on its own)."""
    m, q = A.shape[0], Dt.shape[1]
    G = np.zeros((m, q))
    for r in range(m):
        acc = np.zeros(q)
        for e in range(A.indptr[r], A.indptr[r + 1]):
            acc = acc + A.data[e] * Dt[A.indices[e]]
        G[dst_row[r]] = acc
    return G


@pytest.mark.parametrize("q", lc.SOLVE_Q)
def test_product_is_bit_identical_to_its_definition(env, q):
    """m in {1, 2, R - 1, R, R + 1, 2 R + 1}; row lengths 0, 1, 31, 32, 33, 64, 70 (more than a
    wavefront) among others; non-integer values; a scrambled row map."""
    R, n = lc.ROWS_PER_GROUP, 97
    lengths = np.array([0, 1, 5, 32, 33, 70, 3, 64, 31, 2, 97, 7])
    for m in (1, 2, R - 1, R, R + 1, 2 * R + 1):
        rng = np.random.default_rng([m, q])
        A = nr.random_csr(rng, m, n, np.roll(np.resize(lengths, m), m % 5),
                          lambda g, k: g.standard_normal(k) * np.ldexp(1.0, g.integers(-8, 9, k)))
        Dt = rng.standard_normal((n, q)) * (rng.random((n, q)) < 0.7)
        dst_row = rng.permutation(m)
        G = env.torch.full((m * q,), np.nan, dtype=env.torch.float64, device=env.dv.ctx().device)
        ip, ix, va, dt, dr = (_dev(env, A.indptr, np.int32), _dev(env, A.indices, np.int32),
                              _dev(env, A.data, np.float64), _dev(env, Dt, np.float64),
                              _dev(env, dst_row, np.int32))     # (held until the result is read)
        env.hip.call("ipx_link_spmm", m, n, q, ip.data_ptr(), ix.data_ptr() if A.nnz else None,
                     va.data_ptr() if A.nnz else None, dt.data_ptr(), dr.data_ptr(), G.data_ptr(),
                     env.dv.stream_ptr())
        got = G.cpu().numpy().reshape(q, m).T                 # column-major, leading dimension m
        want = _product_definition(A, Dt, dst_row)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (m, q, bad[:5])


def test_product_in_the_solver_and_f_is_bitwise_symmetric(env):
    """Through the solver, on non-integer values: G against the definition with the solver's own
    D' and row map, E contiguous at the head of each column, F bitwise symmetric."""
    k, mB, q = 9, lc.ROWS_PER_GROUP + 1, 31
    A, rows, e, w = lc.build(k, mB, q, 0.3, True, "middle")
    rng = np.random.default_rng(3)
    A = sps.csr_matrix(A)
    A.data = A.data * rng.uniform(0.5, 1.5, A.nnz)
    with env.proj.wide_band("block-tridiagonal"):
        solver, Ad = _solver(env, A, rows, np.zeros(A.shape[0], np.int64))
    m, n = A.shape
    _, D = lc.split(A, rows)
    Dt = solver.Dt.cpu().numpy().reshape(n, q)
    assert np.array_equal(Dt, D.T)
    G = solver.G.cpu().numpy().reshape(q, m).T
    split = env.lk.split_rows(Ad.pattern, rows)
    assert np.array_equal(G, _product_definition(A, Dt, split.dst_row))
    F = G[mB:]
    assert np.array_equal(F, F.T)
    assert np.array_equal(solver.Y.cpu().numpy().reshape(q, m)[:, mB:], np.zeros((q, q)))


# ------------------------------------------------- 2. solves at the edges of the partial counts
def _inner_bound(env, inner):
    """The inner solver's own asserted bound, in units of u."""
    if isinstance(inner, env.proj.BandedNormalSolver):
        steps = env.lib.ipx_banded_refine_steps(ctypes.c_void_p(inner.handle), None)
        return (C_ITER if steps else C_DIRECT) * (inner.k + 1)
    assert isinstance(inner, env.bt.BlockTridiagonalNormalSolver)
    return C_BLOCK * inner.stats["levels"] * inner.b


def _solver(env, A, rows, e):
    Ad = env.dv.DeviceCSR.from_scipy(nr.pow2_rows(A, e))
    split = env.lk.split_rows(Ad.pattern, rows)
    assert split is not None and split.q == len(rows)
    return env.lk.LinkedRowsNormalSolver(Ad, split), Ad


def check_solve(env, A, rows, e, w, family, inner_bound=None):
    m, q = A.shape[0], len(rows)
    mB = m - q
    keep = np.ones(m, dtype=bool)
    keep[rows] = False
    S = nr.gram_pow2(A, e)
    B_int, _ = lc.split(A, rows)
    Be, De = lc.split(nr.pow2_rows(A, e), rows)
    solver, _ = _solver(env, A, rows, e)
    if inner_bound is None:
        k_B = bc.half_bandwidth(nr.gram_pow2(B_int))
        want_inner = env.proj.BandedNormalSolver if k_B <= env.lib.ipx_banded_kmax() \
            else env.bt.BlockTridiagonalNormalSolver
        assert type(solver.inner) is want_inner, (k_B, type(solver.inner))
        inner_bound = _inner_bound(env, solver.inner)
    assert solver.flag_bits == 0 and not solver.ill_conditioned and solver.perm is None
    # D' as scattered, E and F exactly (integers times powers of two), K against the twin's
    n = A.shape[1]
    assert np.array_equal(solver.Dt.cpu().numpy().reshape(n, q), De.T)
    G = solver.G.cpu().numpy().reshape(q, m).T
    assert np.array_equal(G[:mB], Be @ De.T) and np.array_equal(G[mB:], De @ De.T)
    v_twin, K_twin, F_twin = lc.twin(Be, De, lc.band_first(rows, m, w))
    v_twin = lc.caller_order(rows, m, v_twin)
    kappa_B = nr.scaled_cond(nr.gram_pow2(B_int, e[keep]))
    K_dev = solver.K.cpu().numpy().reshape(q, q)
    low = np.tril_indices(q)
    scale = np.sqrt(np.outer(np.diag(F_twin), np.diag(F_twin)))
    assert np.max(np.abs(K_dev[low] - K_twin[low]) / scale[low]) <= 1e-9
    canc = lc.cancellation(K_twin, F_twin)
    assert abs(solver.cancellation - canc) <= 1e-6 * canc
    x = solver.solve(env.dv.DVec.from_host(w)).to_host()
    assert x.shape == (m,) and np.all(np.isfinite(x))
    assert solver.stats == {"solves": 1, "inner_solves": q + 1}          # (no refinement step)
    eta = nr.backward_error(S, x, w)
    eta_twin = nr.backward_error(S, v_twin, w)
    eta_lap = nr.backward_error(S, lc.lapack_dense(S, w), w)
    bound = 8 * lc.C_TWIN_LINK * kappa_B + inner_bound
    print("eta/u %-40s %.3g  (twin %.3g, LAPACK dense Cholesky %.3g; bound %.3g: kappa_B %.3g, "
          "max F_jj/K_jj %.3g)" % (family, eta / U, eta_twin / U, eta_lap / U, bound, kappa_B, canc))
    key = family.split(":")[0]
    SEEN[key] = max(SEEN.get(key, (0.0, 0.0)), (eta / (bound * U), eta / U))
    assert eta <= bound * U, (family, eta / U, bound)
    return solver


@pytest.mark.parametrize("k", lc.SOLVE_K)
def test_solve_by_exact_residual(env, k):
    """m_B in {1, 2, R - 1, R, R + 1, 2 R + 1} (R = ipx_border_rows_per_group()), q in
    {1, 2, 31, 32}, link rows at the top, in the middle and at the bottom, fill 1.0 / 0.3, graded
    (2^e, e in [-30, 30]) and plain rows; inner banded (k = 1, 4) and block tridiagonal (k = 9,
    17, from m_B > 8 on)."""
    with env.proj.wide_band("block-tridiagonal" if k > 8 else "iterative"):
        for mB, q, fill, graded, where in lc.solve_cases(k):
            A, rows, e, w = lc.build(k, mB, q, fill, graded, where)
            check_solve(env, A, rows, e, w, "k%d:m_B%d q%d fill%.1f%s %s"
                        % (k, mB, q, fill, " graded" if graded else "", where))


# ------------------------------------------------------------------ 3. nearly dependent rows
def test_nearly_dependent_link_rows(env):
    """Link rows that are combinations of band rows up to +-1 on three columns: F_jj / K_jj in
    the thousands, the same bound, no refinement (check_solve asserts the counters)."""
    A, rows, e, w = lc.nearly_dependent_case()
    with env.proj.wide_band("block-tridiagonal"):
        solver = check_solve(env, A, rows, e, w, "nearly:k9")
    assert solver.cancellation > 100
    assert isinstance(solver.inner, env.bt.BlockTridiagonalNormalSolver)


# ------------------------------------------------------------------------------- 4. guards
def _name_or_error(proj, Ad):
    """What the selection hands out for a matrix: the solver's name, or how it refuses."""
    try:
        return proj.solver_name(proj.normal_solver_for(Ad))
    except np.linalg.LinAlgError:
        return "LinAlgError"


@pytest.mark.parametrize("case", ["identical-link-rows", "identical-band-rows"])
def test_guards_fall_back_to_todays_solver(env, case):
    proj, dv = env.proj, env.dv
    A, rows = {"identical-link-rows": lc.identical_link_rows_case,
               "identical-band-rows": lc.identical_band_rows_case}[case]()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with proj.wide_band("block-tridiagonal"):
            today = _name_or_error(proj, dv.DeviceCSR.from_scipy(A))
            Ad = dv.DeviceCSR.from_scipy(A)
            split = env.lk.split_rows(Ad.pattern, rows)
            with proj.link_rows(4):
                assert proj._link_split_for(Ad.pattern) is not None
            try:
                solver = env.lk.LinkedRowsNormalSolver(Ad, split)
            except env.lk.LinkedRefused as exc:
                assert ("B B'" in str(exc)) == (case == "identical-band-rows")
            else:
                # the last pivot of K came out positive and tiny: the soft bit, which the
                # selection treats as a refusal too
                assert case == "identical-link-rows" and solver.ill_conditioned
                assert solver.flag_bits & 1
            with proj.link_rows(4):
                got = _name_or_error(proj, Ad)
    assert "Linked" not in got and got == today, (got, today)


def test_exactly_singular_k_is_not_solved_silently(env):
    """A link row that is an exact integer combination of band rows: refused, or flagged."""
    A, rows, e, w = lc.nearly_dependent_case(noise=False)
    with env.proj.wide_band("block-tridiagonal"):
        try:
            solver, _ = _solver(env, A, rows, e)
        except env.lk.LinkedRefused:
            return
    assert solver.ill_conditioned and solver.flag_bits & 1
    assert solver.cancellation > 2.0 ** 43


# ------------------------------------------------------------ 5. uniform scaling is exact
def test_uniform_scaling_is_exact(env):
    """Rows scaled by 2^s (block-tridiagonal inner, exactly equivariant by its own test): Y does
    not change, K scales by 4^s and, for the same w, v by 4^-s -- bit for bit."""
    k, mB, q = 9, lc.ROWS_PER_GROUP + 1, 3
    A, rows, e0, w = lc.build(k, mB, q, 0.3, True, "middle")

    def run(s):
        solver, _ = _solver(env, A, rows, e0 + s)
        assert isinstance(solver.inner, env.bt.BlockTridiagonalNormalSolver)
        v = solver.solve(env.dv.DVec.from_host(w)).to_host()
        return solver.K.cpu().numpy(), solver.Y.cpu().numpy(), v, solver.cancellation

    with env.proj.wide_band("block-tridiagonal"):
        K0, Y0, v0, c0 = run(0)
        for s in (-37, 41):
            K, Y, v, c = run(s)
            assert np.array_equal(np.ldexp(K, -2 * s), K0) and c == c0
            assert np.array_equal(Y, Y0)
            bad = np.flatnonzero(np.ldexp(v, 2 * s) != v0)
            assert len(bad) == 0, (s, bad[:5])


# ------------------------------------------------------------------------- 6. determinism
def test_factorization_and_solve_are_deterministic(env):
    k, mB, q = 9, 2 * lc.ROWS_PER_GROUP + 1, 31
    A, rows, e, w = lc.build(k, mB, q, 1.0, True, "top")
    with env.proj.wide_band("block-tridiagonal"):
        (one, _), (two, _) = (_solver(env, A, rows, e) for _ in range(2))
    m, n = A.shape
    cnt = n * q + 2 * m * q + 2 * q * q + 2                 # D', G, Y, K, L, info
    assert np.array_equal(one.ws[:cnt].cpu().numpy(), two.ws[:cnt].cpu().numpy())
    wd = env.dv.DVec.from_host(w)
    xs = [one.solve(wd).to_host(), one.solve(wd).to_host(), two.solve(wd).to_host()]
    assert np.array_equal(xs[0], xs[1]) and np.array_equal(xs[0], xs[2])


# ------------------------------------------------------- 7. link rows and border columns
def test_composition_with_border_columns(env):
    """``bd.staged_problem_with_parameters(npar=2)`` (its values times 64, the parameter columns
    rounded to integers: the exact residual needs them) plus two link rows, under all three
    options: linked on bordered on block tridiagonal, eta within the sum of the two bounds."""
    proj = env.proj
    J, _, _ = bd.staged_problem_with_parameters(npar=2)
    Ji = sps.csr_matrix(J * 64.0)
    Ji.data = np.where(np.round(Ji.data) == 0, 1.0, np.round(Ji.data))
    cols = J.shape[1] - 2 + np.arange(2)
    rng = np.random.default_rng(11)
    A, rows = lc.linked(rng, Ji, 2, 1.0, 2 ** 6, "middle")
    A, rows, e, w = lc._finish(rng, A, rows, False)
    B_int, _ = lc.split(A, rows)
    BB, C = bd.split(B_int, cols)
    _, K_b = bd.twin(BB, C, np.ones(B_int.shape[0]))
    with proj.wide_band("block-tridiagonal"), proj.border_columns(4), proj.link_rows(4):
        Ad = env.dv.DeviceCSR.from_scipy(A)
        split = proj._link_split_for(Ad.pattern)
        assert split is not None and np.array_equal(split.d_rows, rows)
        solver = proj.normal_solver_for(Ad)
        name = "LinkedRowsNormalSolver/BorderedNormalSolver/BlockTridiagonalNormalSolver"
        assert proj.last_normal_solver() == name and proj.solver_name(solver) == name
        bordered_bound = 8 * bd.C_TWIN * nr.scaled_cond(nr.gram_pow2(BB)) * float(np.trace(K_b)) \
            + _inner_bound(env, solver.inner.inner)
        check_solve(env, A, rows, e, w, "composed:staged", inner_bound=bordered_bound)


# -------------------------------------------------------- 8. projections against the oracle
def test_projections_against_the_oracle(env):
    import oracle
    from ipsolver import cg_fused
    proj, dv = env.proj, env.dv
    A, _, _, rows = lc.staged_problem_with_links()
    m, n = A.shape
    rng = np.random.default_rng(7)
    Zo, LSo, Yo = oracle.projections(A)
    x, b = rng.standard_normal(n), rng.standard_normal(m)
    Ad = dv.DeviceCSR.from_scipy(A)
    rel = lambda a, want: np.max(np.abs(a - want)) / max(1.0, np.max(np.abs(want)))
    name = "LinkedRowsNormalSolver/BlockTridiagonalNormalSolver"
    with proj.wide_band("block-tridiagonal"), proj.link_rows(8):
        Z, LS, Y = proj.projections(Ad)
        solver = Z.projector.solver
        assert isinstance(solver, proj.LinkedRowsNormalSolver) and 1 <= solver.q <= len(rows)
        assert proj.last_normal_solver() == name
        z = Z.dot(x).to_host()
        assert rel(z, Zo.dot(x)) <= 1e-10
        assert rel(LS.dot(x).to_host(), LSo.dot(x)) <= 1e-10
        assert rel(Y.dot(b).to_host(), Yo.dot(b)) <= 1e-10
        assert np.linalg.norm(A @ z) <= 1e-12 * scipy.sparse.linalg.norm(A) * np.linalg.norm(z)
        assert cg_fused._solver_kind(solver) is None          # the host-driven loop
        proj._last_solver[0] = None
        assert proj.projections(Ad)[0] is Z                   # a reused factorization is named
        assert proj.last_normal_solver() == name
    # outside the context: a new factorization (the limit is part of the cache key), today's
    assert proj.link_rows_limit() == 0
    with proj.wide_band("block-tridiagonal"):
        Z2, _, _ = proj.projections(Ad)
        assert Z2 is not Z and "Linked" not in proj.last_normal_solver()


# --------------------------------------------------------------- 9. through the public call
@pytest.mark.parametrize("inequality", [False, True])
def test_public_call_with_the_link_rows_option(env, inequality):
    """The staged problem of the block-tridiagonal test with a periodicity block and a budget
    row: as an equality without a box, and as an inequality with a box on every variable; the
    same solution with and without the option, ``normal_solver`` naming the linked solver."""
    import ipsolver
    if inequality:
        J, rhs, target, _, budget, cap = lc.staged_problem_with_links(inequality=True)
    else:
        J, rhs, target, _ = lc.staged_problem_with_links()
    n = J.shape[1]

    def solve(options):
        zero = lambda x, v: sps.csr_matrix((n, n))
        cons = [ipsolver.NonlinearConstraint(lambda x: J @ x - rhs, ("equals", 0), lambda x: J,
                                             zero)]
        if inequality:
            cons.append(ipsolver.NonlinearConstraint(lambda x: budget @ x - cap, ("less", 0),
                                                     lambda x: budget, zero))
            cons.append(ipsolver.BoxConstraint(("interval", -2.0, 2.0)))
        return ipsolver.minimize_constrained(
            lambda x: 0.5 * float((x - target) @ (x - target)), np.zeros(n),
            lambda x: x - target, lambda x: sps.identity(n, format="csr"), cons,
            options=options)

    linked = solve({"wide_band": "block-tridiagonal", "link_rows": 8})
    default = solve({})
    assert env.proj.link_rows_limit() == 0 and env.proj.wide_band_policy() == "iterative"
    assert linked.status in (1, 2) and default.status in (1, 2), (linked.status, default.status)
    print("normal_solver: %s (linked), %s (default); niter %d / %d"
          % (linked.normal_solver, default.normal_solver, linked.niter, default.niter))
    assert np.max(np.abs(linked.x - default.x)) <= 1e-6
    assert np.max(np.abs(J @ linked.x - rhs)) <= 1e-7
    want = "BoxSchurNormalSolver/LinkedRowsNormalSolver" if inequality else "LinkedRowsNormalSolver"
    assert linked.normal_solver.startswith(want + "/"), linked.normal_solver
    assert isinstance(default.normal_solver, str) and "Linked" not in default.normal_solver
    with pytest.raises(ValueError, match="link_rows"):
        solve({"link_rows": 33})
