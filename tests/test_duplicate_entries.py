"""Repeated (row, column) entries in a user's CSR Jacobian: scipy defines them as summed, and
the constraint wrappers hand on the canonical matrix (a copy; the caller's stays as it was).
Host only."""
import numpy as np
import scipy.sparse as sps

import normal_ref as nr
from ipsolver import constraints as cs


def _dup_matrix(seed=0):
    rng = np.random.default_rng(seed)
    A = nr.random_csr(rng, 40, 90, rng.integers(0, 9, 40), nr.bits26_values)
    D = nr.split_duplicates(A)
    # one repeat out of order and one entry split three ways, too
    D = sps.csr_matrix((np.concatenate((D.data, [1.5, 0.25, -0.75])),
                        np.concatenate((D.indices, [3, 7, 3])),
                        np.concatenate((D.indptr, [D.indptr[-1] + 3]))), shape=(41, 90))
    return A, D


def _state(M):
    return M.data.copy(), M.indices.copy(), M.indptr.copy()


def _unchanged(M, st):
    return all(np.array_equal(a, b) for a, b in zip(st, (M.data, M.indices, M.indptr)))


def test_canonical_csr_sums_on_a_copy():
    A, D = _dup_matrix()
    st = _state(D)
    C = cs.canonical_csr(D)
    assert C.has_canonical_format and C is not D
    assert np.array_equal(C.toarray(), D.toarray())
    assert np.array_equal(C[:40].toarray(), A.toarray())
    assert C.nnz == A.nnz + 2                         # (41, 3) and (41, 7)
    assert C[40, 3] == 0.75 and C[40, 7] == 0.25
    assert _unchanged(D, st)


def test_canonical_csr_passes_canonical_input_through():
    A, _ = _dup_matrix(1)
    assert A.has_canonical_format
    C = cs.canonical_csr(A)
    assert np.shares_memory(C.data, A.data) and np.shares_memory(C.indices, A.indices)
    # other formats: converted (COO sums its repeats on the way)
    coo = sps.coo_matrix(([1.0, 2.0, 4.0], ([0, 0, 1], [2, 2, 0])), shape=(2, 3))
    C = cs.canonical_csr(coo)
    assert C.has_canonical_format and np.array_equal(C.toarray(), [[0, 0, 3], [4, 0, 0]])


def test_nonlinear_constraint_jacobian_is_canonical():
    A, D = _dup_matrix(2)
    st = _state(D)
    con = cs.NonlinearConstraint(lambda x: D.dot(x), ("less", 10.0), lambda x: D)
    con.evaluate_and_initialize(np.zeros(90))
    for J in (con.J0, con.jac(np.ones(90))):
        assert sps.isspmatrix_csr(J) and J.has_canonical_format
        assert np.array_equal(J.toarray(), D.toarray())
    assert _unchanged(D, st)


def test_linear_constraint_matrix_is_canonical():
    A, D = _dup_matrix(3)
    st = _state(D)
    con = cs.LinearConstraint(D, ("less", 10.0))
    con.evaluate_and_initialize(np.zeros(90))
    assert con.A.has_canonical_format and con.J0 is con.A
    assert np.array_equal(con.A.toarray(), D.toarray())
    assert _unchanged(D, st)
    nl = con.to_nonlinear()
    assert nl.jac(np.zeros(90)).has_canonical_format


def test_sparse_jacobian_from_a_dense_first_value_is_canonical():
    """sparse_jacobian=True with a callback that returns duplicates after a dense J0."""
    A, D = _dup_matrix(4)
    con = cs.NonlinearConstraint(lambda x: D.dot(x), ("less", 10.0),
                                 lambda x: D if x[0] else D.toarray())
    con.evaluate_and_initialize(np.zeros(90), sparse_jacobian=True)
    assert con.J0.has_canonical_format
    J = con.jac(np.ones(90))
    assert J.has_canonical_format and np.array_equal(J.toarray(), D.toarray())


def test_references_agree():
    """The two exact references of tests/normal_ref.py on the same integer-valued input."""
    rng = np.random.default_rng(6)
    A = nr.random_csr(rng, 70, 50, rng.integers(0, 8, 70), nr.int_values)
    w = nr.int_values(rng, 50, 2 ** 6)
    perm = rng.permutation(70)
    for wcol in (None, w):
        S = nr.aat_int(A, wcol)
        B = A.multiply(wcol[None, :]) if wcol is not None else A
        assert np.array_equal(S, B.dot(A.T).toarray())
        for p in (None, perm):
            val, mag, cnt = nr.band_fsum(A, p, 4, wcol)
            assert np.array_equal(val, nr.band_of(S, p, 4))
            assert np.all(mag >= np.abs(val)) and cnt.max() > 1
    D = A.toarray()
    val, mag = nr.gram_fsum_dense(D)
    assert np.array_equal(val, nr.gram_int(D))
    v2, _, _ = nr.gram_fsum_csr(A)
    assert np.array_equal(v2, val)
    # the bound: exact for one product, gamma_k scaled otherwise
    assert nr.within_bound(1.0, 1.0, 1.0, 1) and not nr.within_bound(1.0 + 2 ** -52, 1.0, 1.0, 1)
    assert nr.within_bound(1.0 + 2 ** -52, 1.0, 1.0, 3)
