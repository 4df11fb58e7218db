"""The device exit for rank-deficient sparse Jacobians (``sparse_rank_deficient = "skip-pivots"``:
csrc/nested.hip / csrc/dense.hip in skip mode, ipsolver/nested.py ``PivotSkippingNestedSolver``,
ipsolver/sparse_deficient.py).

  1. solver level, on every case of tests/sparse_deficient_cases.py (both front paths, the skipped
     pivot at every place tests/test_sparse_deficient_host.py asserts): the dropped rows are the
     numpy model's, ``K+ w`` is exactly 0 there and, on the kept rows, a solve with ``A_S A_S'``
     judged by the exact residual of tests/normal_ref.py -- bound C_ND of
     tests/test_gpu_nested_dissection.py over LAPACK's Cholesky of that same matrix;
  2. skip mode on a full-rank matrix: the fronts bit for bit the normal mode's; determinism;
  3. Z, LS, Y from ``projections`` against the oracle's SVD operators: relative max-norm error
     <= 50 kappa eps, kappa = max(sigma_1 / sigma_rank(A), cond(A_S)), A_S the rows the MODEL
     keeps (the method's error follows cond(A_S); both are printed);
  4. routing: the warning, the host exit without the option, past 32 dropped rows and for
     ``method="SVDFactorization"``.
Everything here fails on the parent commit: the option's name is unknown there.
"""
import warnings

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sps
import scipy.sparse.linalg

import normal_ref as nr
import sparse_deficient_cases as cases
import test_gpu_nested_dissection as nd

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
OPTION = {"sparse_rank_deficient": "skip-pivots"}
WARNING = ("Singular Jacobian matrix. Using a pivot-skipping sparse Cholesky factorization on "
           "the device to perform the factorizations.")
ORTH_TOL = 1e-12
ENTRY_EXPONENT = -13                    # every entry is an integer times 2^-13 (2^-3 * 2^-10)


def skip_class(leaf, small=None):
    from ipsolver.nested import PivotSkippingNestedSolver
    attrs = {"LEAF": leaf}
    if small is not None:
        attrs["SMALL_FRONT"] = small
    return type("CutSkip", (PivotSkippingNestedSolver,), attrs)


def build_solver(name):
    import ipsolver.device as dv
    A, leaf, small, _, _ = cases.built(name)
    return skip_class(leaf, small)(dv.DeviceCSR.from_scipy(A))


def projections_warned(A, cls=None, method=None, **scopes):
    """``projections(A)`` under the option scopes, the last solver's name, the warnings."""
    import ipsolver.projector as proj
    import ipsolver.solver_options as so
    from ipsolver.sparse_deficient import SparseDeficientProjector as P
    before = P.solver_class
    if cls is not None:
        P.solver_class = cls
    try:
        with so.scoped(**scopes):
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                ops = proj.projections(A, method=method)
            name = proj.last_normal_solver()
    finally:
        P.solver_class = before
    return ops, name, [str(w.message) for w in caught]


# ------------------------------------------------------------------------------ 1. solver level
@pytest.mark.parametrize("name", sorted(cases.all_cases()))
def test_solver_against_the_model(name):
    import ipsolver.device as dv
    A, _, small, sym, mod = cases.built(name)
    m = A.shape[0]
    solver = build_solver(name)
    assert solver.flag_bits == 0 and not solver.ill_conditioned
    assert np.array_equal(solver.dropped, mod.dropped), (solver.dropped, mod.dropped)
    assert solver.rank == m - len(mod.dropped) == mod.rank
    assert np.array_equal(np.flatnonzero(solver.mark.cpu().numpy()), mod.dropped)
    assert (solver.stats["large_fronts"] > 0) == (small is not None)
    assert solver.symbolic is not sym and np.array_equal(solver.symbolic.perm, sym.perm)
    w = np.random.default_rng(m).standard_normal(m)
    x = solver.solve(dv.DVec.from_host(w)).to_host()
    assert np.all(np.isfinite(x))
    assert np.all(x[mod.dropped] == 0.0)
    keep = mod.kept
    Ai = sps.csr_matrix(A[keep] * 2.0 ** -ENTRY_EXPONENT)
    S = nr.gram_pow2(Ai, np.full(len(keep), ENTRY_EXPONENT))
    host = scipy.linalg.cho_solve(scipy.linalg.cho_factor(S.toarray(), lower=True), w[keep])
    nd.check_eta("skip " + name, x[keep], S, w[keep], nr.backward_error(S, host, w[keep]))
    # the right-hand side's entries at the dropped rows are not read
    w2 = w.copy()
    w2[mod.dropped] = 1e300
    assert np.array_equal(solver.solve(dv.DVec.from_host(w2)).to_host(), x)


# ------------------------------------------------------------------------------ 2. bit identity
@pytest.mark.parametrize("name", ["grid48", "grid48-tiled", "random"])
def test_skip_mode_on_a_full_rank_matrix_is_the_normal_mode(name):
    import ipsolver.device as dv
    import torch
    Ai, e, _, w, _ = nd.system(name)
    _, leaf, small, _ = nd.CASES[name]
    normal = nd.build_solver(name)
    skip = skip_class(leaf, small)(dv.DeviceCSR.from_scipy(nr.pow2_rows(Ai, e)))
    assert len(skip.dropped) == 0 and skip.rank == skip.m and skip.flag_bits == 0
    assert torch.equal(normal.ws, skip.ws)
    assert torch.equal(normal.flag, skip.flag)
    wd = dv.DVec.from_host(w)
    assert np.array_equal(normal.solve(wd).to_host(), skip.solve(wd).to_host())


@pytest.mark.parametrize("name", ["lds-two-in-one-front", "tile-64", "appended-sum"])
def test_factorization_and_solve_are_deterministic(name):
    import ipsolver.device as dv
    import torch
    one, two = build_solver(name), build_solver(name)
    assert torch.equal(one.ws, two.ws) and torch.equal(one.mark, two.mark)
    wd = dv.DVec.from_host(np.random.default_rng(3).standard_normal(one.m))
    x1, x2, x3 = one.solve(wd).to_host(), one.solve(wd).to_host(), two.solve(wd).to_host()
    assert np.array_equal(x1, x2) and np.array_equal(x1, x3)


# ------------------------------------------------------------------------------ 3. operators
@pytest.mark.parametrize("name", sorted(cases.all_cases()))
def test_operators_against_the_oracle(name):
    import ipsolver.device as dv
    A, leaf, small, _, mod = cases.built(name)
    m, n = A.shape
    q = len(mod.dropped)
    rng = np.random.default_rng(m + n + q)
    x, b = rng.standard_normal(n), rng.standard_normal(m)
    Zo, LSo, Yo = cases.oracle_svd_operators(A)
    (Z, LS, Y), solver, messages = projections_warned(dv.DeviceCSR.from_scipy(A),
                                                      skip_class(leaf, small), **OPTION)
    assert messages == [WARNING], messages
    assert solver == "CutSkip"
    P = Z.projector
    assert type(P).__name__ == "SparseDeficientProjector"
    assert np.array_equal(P.dropped, mod.dropped) and P.rank == m - q == P.stats["rank"]
    assert P.stats["dropped"] == q
    host = lambda v: v.to_host()
    zx, lsx, yb = host(Z.dot(x)), host(LS.dot(x)), host(Y.dot(b))
    assert P.stats["solves"] >= 3
    cond_A, cond_S = cases.conditions(A, mod.kept)
    tol = 50 * max(cond_A, cond_S) * EPS

    def rel(a, want):
        return np.max(np.abs(a - want)) / np.max(np.abs(want))
    errs = rel(lsx, LSo.dot(x)), rel(yb, Yo.dot(b)), rel(zx, Zo.dot(x))
    orth = np.linalg.norm(A.dot(zx)) / (scipy.sparse.linalg.norm(A) * np.linalg.norm(x))
    print("sparse_deficient operators %s: cond(A) %.1e cond(A_S) %.1e LS %.2e Y %.2e Z %.2e "
          "(tol %.2e) orth %.2e refinements %d dependency residual %.2e"
          % (name, cond_A, cond_S, errs[0], errs[1], errs[2], tol, orth,
             P.stats["refinements"], P.stats["dependency_residual"]))
    assert max(errs) <= tol
    assert orth <= ORTH_TOL


# ------------------------------------------------------------------------------ 4. routing
def test_without_the_option_the_host_exit():
    import ipsolver.device as dv
    import ipsolver.projector as proj
    A = cases.built("lds-leaf-front")[0]
    (Z, _, _), solver, messages = projections_warned(dv.DeviceCSR.from_scipy(A))
    assert isinstance(Z.projector, proj.SVDProjector) and solver == "SVDProjector"
    assert len(messages) == 1 and "dense SVD" in messages[0]
    (Z, _, _), solver, messages = projections_warned(dv.DeviceCSR.from_scipy(A), **OPTION)
    assert solver == "PivotSkippingNestedSolver" and messages == [WARNING]
    assert "dense SVD" not in messages[0]
    assert proj.sparse_rank_deficient_choice() == "host-svd"


def test_more_than_32_dropped_rows_fall_back_to_the_host_exit():
    import ipsolver.device as dv
    import ipsolver.projector as proj
    A = cases.thinned_g()
    (Z, _, _), solver, messages = projections_warned(dv.DeviceCSR.from_scipy(A),
                                                     skip_class(32), **OPTION)
    assert isinstance(Z.projector, proj.SVDProjector) and solver == "SVDProjector"
    assert len(messages) == 1 and "dense SVD" in messages[0]


def test_svd_factorization_keeps_the_host_exit():
    import ipsolver.projector as proj
    A = cases.built("combination")[0].toarray()
    (Z, _, _), solver, messages = projections_warned(A, method="SVDFactorization", **OPTION)
    assert isinstance(Z.projector, proj.SVDProjector) and messages == []


def test_a_full_rank_matrix_does_not_see_the_option():
    import ipsolver.device as dv
    A = cases.full_grid(12)
    (Z, _, _), solver, messages = projections_warned(dv.DeviceCSR.from_scipy(A), **OPTION)
    assert solver == "DenseNormalSolver" and messages == []
