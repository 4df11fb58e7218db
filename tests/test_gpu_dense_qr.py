"""Householder QR projections for dense Jacobians on the device
(``dense_factorization = "householder-qr"``: ipsolver/dense_qr.py, csrc/denseqr.hip).

  1. the factorization against LAPACK's on the same input (orthogonality, backward error,
     diag R, determinism);
  2. the three operators against the oracle (pivoted QR) up to cond(A) = 1e12;
  3. rank-deficient input keeps the SVD exit;
  4. caching and scoping of the option;
  5. end to end: ``tests/test_gpu_dense_qr_e2e.py``.
"""
import warnings

import numpy as np
import pytest

from conftest import host, close

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps

# a single row; square with exactly one panel; panel + 1; two panels + 2 with a ragged n;
# 4 panels; 9 panels (multi-tile trailing updates)
SHAPES = [(1, 5), (64, 64), (65, 300), (130, 700), (200, 1000), (520, 2100)]


@pytest.fixture(scope="module")
def env():
    import ipsolver.device as dv
    import ipsolver.projector as proj
    from ipsolver import dense, dense_qr

    class NS:
        pass
    ns = NS()
    ns.dv, ns.proj, ns.dense, ns.dense_qr = dv, proj, dense, dense_qr
    return ns


def graded(rng, m, n, cond):
    """A = (U logspace(0, -log10 cond, m)) V' (tests/test_gpu_qp.py::test_dense_ill_conditioned)"""
    U, _ = np.linalg.qr(rng.standard_normal((m, m)))
    V, _ = np.linalg.qr(rng.standard_normal((n, m)))
    return (U * np.logspace(0, -np.log10(cond), m)) @ V.T


def identities(A, Q, R):
    m = A.shape[0]
    return (np.max(np.abs(Q.T @ Q - np.eye(m))),
            np.max(np.abs(A.T - Q @ R)) / np.max(np.abs(A)))


def pivot_ratio_numpy(A):
    R = np.linalg.qr(A.T, mode="r")
    return np.min(np.abs(np.diag(R)) / np.linalg.norm(A, axis=1))


@pytest.mark.parametrize("kind", ["normal", "graded"])
@pytest.mark.parametrize("m,n", SHAPES)
def test_factorization_against_lapack(env, m, n, kind):
    if kind == "graded" and m == 1:
        return                      # (one row has no spectrum to grade)
    rng = np.random.default_rng(1000 * m + n)
    A = rng.standard_normal((m, n)) if kind == "normal" else graded(rng, m, n, 1e10)
    D = env.dense.DeviceDense.from_host(A)
    P = env.dense_qr.DenseQRProjector(D)
    Q, R = P.Q_host(), P.R_host()
    assert Q.shape == (n, m) and R.shape == (m, m)
    assert np.all(np.tril(R, -1) == 0.0)
    Ql, Rl = np.linalg.qr(A.T)
    orth, back = identities(A, Q, R)
    orth_l, back_l = identities(A, Ql, Rl)
    print("dense_qr %s (%d, %d): orth %.2f eps (lapack %.2f), backward %.2f eps (lapack %.2f)"
          % (kind, m, n, orth / EPS, orth_l / EPS, back / EPS, back_l / EPS))
    assert orth <= max(16 * EPS, 8 * orth_l)
    assert back <= max(16 * EPS, 8 * back_l)
    ratio = np.abs(np.diag(R)) / np.abs(np.diag(Rl))
    assert np.all(ratio <= 2.0) and np.all(ratio >= 0.5)
    assert 0.5 <= P.pivot_ratio / pivot_ratio_numpy(A) <= 2.0
    # a second factorization of the same matrix: the same bits
    P2 = env.dense_qr.DenseQRProjector(D)
    assert np.array_equal(P2.Q_host(), Q) and np.array_equal(P2.R_host(), R)
    assert P2.pivot_ratio == P.pivot_ratio
    # the stored strict lower part of R is never read: the operators agree with dense
    # products of the factors read back.  (Two ways of solving with the same R: each has a
    # relative forward error of order m eps cond(R); 1e-13 = 450 eps covers the constants.  A
    # stray entry under the diagonal would show at order 1 for the well-conditioned inputs.)
    x, b = rng.standard_normal(n), rng.standard_normal(m)
    ls = np.linalg.solve(R, Q.T @ x)
    y = Q @ np.linalg.solve(R.T, b)
    tol = 1e-13 * np.linalg.cond(R) * m
    assert np.max(np.abs(host(P.least_squares(env.dv.DVec.from_host(x))) - ls)) \
        <= tol * max(1.0, np.max(np.abs(ls)))
    assert np.max(np.abs(host(P.row_space(env.dv.DVec.from_host(b))) - y)) \
        <= tol * max(1.0, np.max(np.abs(y)))
    if m == n:
        # the null space is empty: Z x = 0 up to rounding
        z = host(P.null_space(env.dv.DVec.from_host(x)))
        assert np.max(np.abs(z)) <= 64 * EPS * np.max(np.abs(x))


@pytest.mark.parametrize("cond", [1e3, 1e6, 1e8, 1e10, 1e12])
@pytest.mark.parametrize("m,n", [(200, 1000), (130, 700)])
def test_operators_against_oracle(env, m, n, cond):
    """Z, LS, Y under the option against the oracle's pivoted QR, in the measure and with the
    tolerance of test_dense_ill_conditioned -- without its refinement steps for LS and Y, and
    without the Cholesky path's "Singular Jacobian" exit from cond(A) of about 1e8."""
    import oracle
    rng = np.random.default_rng(int(np.log10(cond)))
    A = graded(rng, m, n, cond)
    x, b = rng.standard_normal(n), rng.standard_normal(m)
    Zo, LSo, Yo = oracle.projections(A)
    with env.proj.dense_factorization("householder-qr"):
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            Z, LS, Y = env.proj.projections(A)
            zx, lsx, yb = Z.dot(x), LS.dot(x), Y.dot(b)
        assert env.proj.last_normal_solver() == "DenseQRProjector"
    P = Z.projector
    assert type(P).__name__ == "DenseQRProjector"

    def rel(a, want):
        return np.max(np.abs(host(a) - want)) / np.max(np.abs(want))
    tol = max(1e-10, 50 * cond * EPS)
    errs = rel(lsx, LSo.dot(x)), rel(yb, Yo.dot(b)), rel(zx, Zo.dot(x))
    orth = env.proj.orthogonality(A, zx)
    print("dense_qr operators (%d, %d) cond %.0e: LS %.2e Y %.2e Z %.2e (tol %.2e) orth %.2e "
          "pivot ratio 2^%.1f refinements %d"
          % (m, n, cond, errs[0], errs[1], errs[2], tol, orth, np.log2(P.pivot_ratio),
             P.stats["refinements"]))
    assert max(errs) <= tol
    assert orth <= 1e-12
    assert 0.5 <= P.pivot_ratio / pivot_ratio_numpy(A) <= 2.0
    assert P.pivot_ratio > 2.0 ** -43
    if cond == 1e10:
        assert P.stats["refinements"] >= 1


@pytest.mark.parametrize("kind", ["duplicate", "combination", "zero"])
@pytest.mark.parametrize("m,n", [(65, 300), (130, 700)])
def test_rank_deficient_keeps_the_svd_exit(env, m, n, kind):
    """The matrix is scaled by 2^-10 (exact) so that the singular value that is zero in exact
    arithmetic -- a few eps ||A||_2 as LAPACK computes it -- lies below the reference's
    tol = 1e-15 for the oracle and for ``SVDProjector`` alike: both then drop it, and the
    operators are those of the rank m - 1 matrix (asserted on the host below)."""
    import oracle
    rng = np.random.default_rng(7 * m + len(kind))
    A = rng.standard_normal((m, n)) * 2.0 ** -10
    r = m - 3
    if kind == "duplicate":
        A[r] = A[5]
    elif kind == "combination":
        A[r] = rng.standard_normal(r) @ A[:r]
    else:
        A[r] = 0.0
    assert np.linalg.svd(A, compute_uv=False)[-1] <= 1e-15
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Zo, LSo, Yo = oracle.projections(A)
    x, b = rng.standard_normal(n), rng.standard_normal(m)
    with env.proj.dense_factorization("householder-qr"):
        with pytest.warns(UserWarning, match="Singular Jacobian"):
            Z, LS, Y = env.proj.projections(A)
    assert type(Z.projector).__name__ == "SVDProjector" and Z.projector.rank == m - 1
    close(Z.dot(x), Zo.dot(x), 1e-10)
    close(LS.dot(x), LSo.dot(x), 1e-9)
    close(Y.dot(b), Yo.dot(b), 1e-10)


def test_caching_and_scoping(env):
    rng = np.random.default_rng(5)
    A = rng.standard_normal((130, 700))
    x = rng.standard_normal(700)
    D = env.dense.DeviceDense.from_host(A)
    Z0, LS0, _ = env.proj.projections(D)
    assert type(Z0.projector.solver).__name__ == "DenseNormalSolver"
    before = host(Z0.dot(x)), host(LS0.dot(x))
    with env.proj.dense_factorization("householder-qr"):
        Z1, _, _ = env.proj.projections(D)
        assert type(Z1.projector).__name__ == "DenseQRProjector"
        assert env.proj.last_normal_solver() == "DenseQRProjector"
        assert env.proj.projections(D)[0] is Z1            # (cached under its own key)
        Z1.dot(x)
    assert env.proj.dense_factorization_choice() == "normal-equations"
    Z2, LS2, _ = env.proj.projections(D)
    assert Z2.projector is not Z1.projector
    assert type(Z2.projector.solver).__name__ == "DenseNormalSolver"
    assert env.proj.last_normal_solver() == "DenseNormalSolver"
    # nothing shared, nothing mutated: the default path's bits are what they were
    assert np.array_equal(host(Z2.dot(x)), before[0])
    assert np.array_equal(host(LS2.dot(x)), before[1])
    assert np.array_equal(D.to_host(), A)
    # a sparse Jacobian ignores the option
    import scipy.sparse as sps
    S = sps.random(40, 200, density=0.2, random_state=3, format="csr") + sps.eye(40, 200)
    with env.proj.dense_factorization("householder-qr"):
        Zs, _, _ = env.proj.projections(S.tocsr())
    assert type(Zs.projector).__name__ == "NormalEquationProjector"
