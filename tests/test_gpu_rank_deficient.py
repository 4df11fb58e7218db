"""Rank-deficient dense Jacobians stay on the device (``rank_deficient = "pivoted-qr"``:
ipsolver/dense_cod.py, csrc/denseqrp.hip).  Inputs: tests/rank_deficient_cases.py, whose
conditions tests/test_rank_deficient_host.py asserts.

  1. the column-pivoted factorization: permutation, rank, the pivoting inequality, and
     orthogonality / backward error against LAPACK's pivoted QR truncated at the same rank;
  2. the three operators against the oracle (whose SVD exit drops the same singular values);
  3. both ways in: the default dense factorization and the Householder QR;
  4. nothing else moves: full-rank input, sparse input, m > n, caching;
  5. end to end: ``tests/test_gpu_rank_deficient_e2e.py``.
"""
import warnings

import numpy as np
import pytest
import scipy.linalg

from conftest import host, close
import rank_deficient_cases as cases

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
OPTION = "pivoted-qr"
WARNING = "Singular Jacobian matrix. Using a pivoted QR decomposition on the device"


@pytest.fixture(scope="module")
def env():
    import ipsolver.device as dv
    import ipsolver.projector as proj
    from ipsolver import dense, dense_cod

    class NS:
        pass
    ns = NS()
    ns.dv, ns.proj, ns.dense, ns.dense_cod = dv, proj, dense, dense_cod
    return ns


def projections_warned(env, A, **scopes):
    """``projections(A)`` under the given option scopes and the messages of its warnings."""
    import ipsolver.solver_options as so
    with so.scoped(**scopes):
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            ops = env.proj.projections(A)
        name = env.proj.last_normal_solver()
    return ops, name, [str(w.message) for w in caught]


@pytest.mark.parametrize("name,args", cases.all_cases())
def test_factorization(env, name, args):
    A, rank = cases.build(*args)
    m, n = A.shape
    D = env.dense.DeviceDense.from_host(A)
    P = env.dense_cod.DenseCODProjector(D)
    perm, R, Q1 = P.perm_host(), P.R_host(), P.Q1_host()
    assert np.array_equal(np.sort(perm), np.arange(m))
    assert P.rank == rank
    assert R.shape == (rank, m) and Q1.shape == (n, rank)
    gap = P.pivot_gap
    # a second factorization of the same matrix: the same bits
    P2 = env.dense_cod.DenseCODProjector(D)
    assert P2.rank == rank and np.array_equal(P2.perm_host(), perm)
    assert np.array_equal(P2.R_host(), R) and np.array_equal(P2.Q1_host(), Q1)
    if rank == 0:
        assert gap == (0.0, 0.0)
        print("dense_cod %s: rank 0" % name)
        return
    assert np.all(np.tril(R[:, :rank], -1) == 0.0)
    d = np.abs(np.diag(R))
    assert gap[0] == d[-1] / d[0] and gap[0] > 2.0 ** -43 >= gap[1]
    # |diag R| does not increase.  R_jj^2 and the squared norm the pivot search compared are sums
    # of the same at most n squares in two orders: they differ by n eps at the most.
    assert np.all(d[1:] <= d[:-1] * (1.0 + n * EPS))
    # the pivoting inequality R_jj^2 >= sum_{i = j .. k} R_ik^2 for all k > j, with LAPACK's
    # relative slack sqrt(eps) (tol3z of dlaqp2); S[j, k] = sum_{i >= j} R_ik^2
    S = np.cumsum((R * R)[::-1], axis=0)[::-1]
    excess = S / (d * d)[:, None] - 1.0
    excess[np.tril_indices(rank, 0, m)] = -1.0
    # orthogonality and the truncated backward error against LAPACK's on the same input
    Ql, Rl, Pl = scipy.linalg.qr(A.T, pivoting=True, mode="economic")
    Ql, Rl = Ql[:, :rank], Rl[:rank]
    amax = np.max(np.abs(A))
    orth = np.max(np.abs(Q1.T @ Q1 - np.eye(rank)))
    back = np.max(np.abs(A.T[:, perm] - Q1 @ R)) / amax
    orth_l = np.max(np.abs(Ql.T @ Ql - np.eye(rank)))
    back_l = np.max(np.abs(A.T[:, Pl] - Ql @ Rl)) / amax
    print("dense_cod %s: rank %d, pivot gap 2^%.1f | 2^%.1f, orth %.2f eps (lapack %.2f), "
          "backward %.2f eps (lapack %.2f), pivoting inequality excess %+.1e (relative)"
          % (name, rank, np.log2(gap[0]), np.log2(gap[1]) if gap[1] > 0 else -np.inf,
             orth / EPS, orth_l / EPS, back / EPS, back_l / EPS, np.max(excess)))
    assert np.max(excess) <= np.sqrt(EPS)
    assert orth <= max(16 * EPS, 8 * orth_l)
    assert back <= max(16 * EPS, 8 * back_l)


@pytest.mark.parametrize("name,args", cases.all_cases())
def test_operators_against_oracle(env, name, args):
    """LS, Y, Z in the measure of tests/test_gpu_dense_qr.py::test_operators_against_oracle:
    relative max-norm error <= max(1e-10, 50 cond_r eps), cond_r = sigma_1 / sigma_r of the kept
    part."""
    import oracle
    A, rank = cases.build(*args)
    m, n = A.shape
    rng = np.random.default_rng(m + n + rank)
    x, b = rng.standard_normal(n), rng.standard_normal(m)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Zo, LSo, Yo = oracle.projections(A)
    (Z, LS, Y), solver, messages = projections_warned(env, A, rank_deficient=OPTION)
    assert len(messages) == 1 and messages[0].startswith(WARNING), messages
    assert solver == "DenseCODProjector"
    P = Z.projector
    assert type(P).__name__ == "DenseCODProjector" and P.rank == rank
    zx, lsx, yb = Z.dot(x), LS.dot(x), Y.dot(b)
    orth = env.proj.orthogonality(A, zx)
    if rank == 0:
        assert np.all(host(lsx) == 0.0) and np.all(host(yb) == 0.0)
        assert np.array_equal(host(zx), x)
        assert orth == 0
        return
    cond_r = cases.kept_condition(A, rank)

    def rel(a, want):
        return np.max(np.abs(host(a) - want)) / np.max(np.abs(want))
    tol = max(1e-10, 50 * cond_r * EPS)
    errs = rel(lsx, LSo.dot(x)), rel(yb, Yo.dot(b)), rel(zx, Zo.dot(x))
    print("dense_cod operators %s: cond_r %.1e LS %.2e Y %.2e Z %.2e (tol %.2e) orth %.2e "
          "refinements %d" % (name, cond_r, errs[0], errs[1], errs[2], tol, orth,
                              P.stats["refinements"]))
    assert max(errs) <= tol
    assert orth <= 1e-12


@pytest.mark.parametrize("factorization", ["normal-equations", "householder-qr"])
def test_both_ways_in(env, factorization):
    """The same duplicate-row matrix through the default dense factorization (a lost Cholesky
    pivot) and through the Householder QR (its pivot ratio).  Without the option both take the
    host SVD -- the control, which passes without the option's code -- with it both stay on the
    device, and the two exits agree to the bounds of test_rank_deficient_keeps_the_svd_exit."""
    A, rank = cases.build("duplicate", 65, 300)
    rng = np.random.default_rng(3)
    x, b = rng.standard_normal(300), rng.standard_normal(65)
    (Zs, LSs, Ys), solver, messages = projections_warned(env, A, dense_factorization=factorization)
    assert solver == "SVDProjector" and Zs.projector.rank == rank
    assert len(messages) == 1 and "Using SVD decomposition" in messages[0], messages
    (Z, LS, Y), solver, messages = projections_warned(env, A, dense_factorization=factorization,
                                                      rank_deficient=OPTION)
    assert solver == "DenseCODProjector" and Z.projector.rank == rank
    assert len(messages) == 1 and messages[0].startswith(WARNING), messages
    close(Z.dot(x), host(Zs.dot(x)), 1e-10)
    close(LS.dot(x), host(LSs.dot(x)), 1e-9)
    close(Y.dot(b), host(Ys.dot(b)), 1e-10)


@pytest.mark.parametrize("factorization,solver_name",
                         [("normal-equations", "DenseNormalSolver"),
                          ("householder-qr", "DenseQRProjector")])
def test_full_rank_input_is_untouched(env, factorization, solver_name):
    rng = np.random.default_rng(5)
    A = rng.standard_normal((130, 700))
    x, b = rng.standard_normal(700), rng.standard_normal(130)
    D = env.dense.DeviceDense.from_host(A)
    (Z0, LS0, Y0), name0, messages0 = projections_warned(env, D, dense_factorization=factorization)
    before = host(Z0.dot(x)), host(LS0.dot(x)), host(Y0.dot(b))
    (Z1, LS1, Y1), name1, messages1 = projections_warned(env, D, dense_factorization=factorization,
                                                         rank_deficient=OPTION)
    assert name0 == name1 == solver_name and not messages0 and not messages1
    assert Z1.projector is not Z0.projector             # (factored again under the option's key)
    assert np.array_equal(host(Z1.dot(x)), before[0])
    assert np.array_equal(host(LS1.dot(x)), before[1])
    assert np.array_equal(host(Y1.dot(b)), before[2])


def test_sparse_and_tall_input_keep_the_host_exit(env):
    import scipy.sparse as sps
    rng = np.random.default_rng(11)
    S = sps.random(40, 200, density=0.2, random_state=3, format="lil")
    S[37] = S[5]
    (Z, _, _), name, messages = projections_warned(env, S.tocsr(), rank_deficient=OPTION)
    assert name == "SVDProjector" and type(Z.projector).__name__ == "SVDProjector"
    assert len(messages) == 1 and "Using dense SVD decomposition" in messages[0], messages
    T = rng.standard_normal((30, 20))
    (Z, _, _), name, messages = projections_warned(env, T, rank_deficient=OPTION)
    assert name == "SVDProjector" and Z.projector.rank == 20
    assert len(messages) == 1 and "Using SVD decomposition" in messages[0], messages
    # method="SVDFactorization" is the caller's choice: no warning, the host SVD
    A, rank = cases.build("duplicate", 65, 300)
    with env.proj.rank_deficient(OPTION):
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            Z, _, _ = env.proj.projections(A, method="SVDFactorization")
    assert type(Z.projector).__name__ == "SVDProjector" and Z.projector.rank == rank


def test_caching_and_scoping(env):
    A, rank = cases.build("combination", 65, 300)
    D = env.dense.DeviceDense.from_host(A)
    with env.proj.rank_deficient(OPTION):
        with pytest.warns(UserWarning, match="pivoted QR decomposition on the device"):
            Z1, _, _ = env.proj.projections(D)
        assert type(Z1.projector).__name__ == "DenseCODProjector"
        with warnings.catch_warnings():
            warnings.simplefilter("error")                  # (cached: nothing is factored)
            assert env.proj.projections(D)[0] is Z1
        assert env.proj.last_normal_solver() == "DenseCODProjector"
    assert env.proj.rank_deficient_choice() == "host-svd"
    with pytest.warns(UserWarning, match="Using SVD decomposition"):
        Z2, _, _ = env.proj.projections(D)
    assert Z2 is not Z1 and type(Z2.projector).__name__ == "SVDProjector"
    assert np.array_equal(D.to_host(), A)
