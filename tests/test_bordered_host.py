"""Host side of the bordered solver (ipsolver/bordered.py): the pattern analysis, the inputs of
tests/test_gpu_bordered.py and the numpy twin whose error sets C_TWIN.  No GPU."""
import numpy as np
import pytest
import scipy.sparse as sps

import blocktri_cases as bc
import bordered_cases as bd
import normal_ref as nr

U = nr.U


def _pattern(A):
    from ipsolver.bordered import HostPattern
    A = sps.csr_matrix(A)
    A.sort_indices()
    return HostPattern(A.indptr, A.indices, A.shape)


def _split(A, reach, limit):
    from ipsolver.bordered import border_split
    return border_split(_pattern(A), reach, limit)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("k,reach,p", [(1, 8, 1), (4, 8, 3), (9, 64, 2)])
def test_border_split_chooses_exactly_the_appended_columns(where, k, reach, p):
    rng = np.random.default_rng([k, p])
    base = bc.band_rows(rng, 90, k, lim=2 ** 4)
    A, cols = bd.bordered(rng, base, p, 1.0, 2 ** 4, where=where)
    s = _split(A, reach, 4)
    assert s is not None and np.array_equal(s.cols, cols) and s.p == p and s.k == k
    # the index lists reproduce B and C
    A = sps.csr_matrix(A)
    B, C = bd.split(A, cols)
    got_B = sps.csr_matrix((A.data[s.b_src], s.host.indices_h, s.host.indptr_h), shape=A.shape)
    assert abs(got_B - B).nnz == 0
    got_C = np.zeros(A.shape[0] * p)
    got_C[s.c_dst] = A.data[s.c_src]
    assert len(np.unique(s.c_dst)) == len(s.c_dst)
    assert np.array_equal(got_C.reshape(p, -1).T, C)
    # cached on the pattern, per (reach, limit)
    from ipsolver.bordered import border_split
    pat = _pattern(A)
    assert border_split(pat, reach, 4) is border_split(pat, reach, 4)


def test_border_split_sparse_columns_and_ocp_rows():
    rng = np.random.default_rng(3)
    A, cols = bd.bordered(rng, bc.ocp_rows(12, 4, 40, rng), 3, 0.3, 2 ** 6)
    assert _split(A, 8, 4) is None                      # the band has half bandwidth 23
    s = _split(A, 64, 4)
    assert s is not None and np.array_equal(s.cols, cols) and s.k == 23


def test_border_split_returns_none():
    rng = np.random.default_rng(5)
    base = bc.band_rows(rng, 90, 4, lim=2 ** 4)
    assert _split(base, 8, 4) is None                                   # p = 0
    A, _ = bd.bordered(rng, base, 3, 1.0, 2 ** 4)
    assert _split(A, 8, 2) is None and _split(A, 8, 0) is None          # p > limit
    assert _split(A, 8, 3) is not None
    A, _ = bd.border_only_row_case()
    assert _split(A, 64, 4) is None                                     # a border-only row
    A9, _ = bd.bordered(rng, bc.band_rows(rng, 90, 9, lim=2 ** 4), 1, 1.0, 2 ** 4)
    assert _split(A9, 8, 4) is None                                     # B's k = 9 > reach
    assert _split(A9, 64, 4) is not None
    # a dense column no longer than the reach is not a border
    short, _ = bd.bordered(rng, bc.band_rows(rng, 40, 9, lim=2 ** 4), 1, 1.0, 2 ** 4)
    assert _split(short, 64, 4) is None


def test_border_split_does_not_depend_on_the_order_of_the_other_columns():
    rng = np.random.default_rng(6)
    A, cols = bd.bordered(rng, bc.band_rows(rng, 120, 4, lim=2 ** 4), 2, 0.3, 2 ** 4, where="middle")
    A = sps.csc_matrix(A)
    n = A.shape[1]
    perm = rng.permutation(n)
    Ap = sps.csr_matrix(A[:, perm])
    s, sp = _split(A, 8, 4), _split(Ap, 8, 4)
    assert s is not None and sp is not None
    assert np.array_equal(np.sort(perm[sp.cols]), cols) and sp.k == s.k == 4
    Bp = sps.csr_matrix((Ap.data[sp.b_src], sp.host.indices_h, sp.host.indptr_h), shape=Ap.shape)
    B, _ = bd.split(A, cols)
    assert abs(Bp @ Bp.T - B @ B.T).nnz == 0


def test_option_plumbing():
    from ipsolver import projector
    import ipsolver
    assert projector.border_columns_limit() == 0
    for bad in (-1, bd.P_MAX + 1, 1.5, "4", True):
        with pytest.raises(ValueError, match="border_columns"):
            with projector.border_columns(bad):
                pass
    assert projector._hip.load().ipx_border_pmax() == bd.P_MAX
    assert projector._hip.load().ipx_border_rows_per_group() == bd.ROWS_PER_GROUP
    with pytest.raises(RuntimeError):
        with projector.border_columns(4):
            assert projector.border_columns_limit() == 4
            assert projector.border_reach() == projector._hip.load().ipx_banded_kmax()
            with projector.wide_band("block-tridiagonal"), projector.border_columns(0):
                assert projector.border_columns_limit() == 0
                assert projector.border_reach() == 64
            raise RuntimeError("inside")
    assert projector.border_columns_limit() == 0
    calls = []
    with pytest.raises(ValueError, match="border_columns"):
        ipsolver.minimize_constrained(lambda x: calls.append(1) or 0.0, np.zeros(2),
                                      lambda x: np.zeros(2), options={"border_columns": 33})
    assert not calls


def test_solver_name_recurses_through_inner():
    from ipsolver import projector

    class Leaf:
        pass

    class Mid:
        inner = Leaf()

    class Outer:
        inner = Mid()
    assert projector.solver_name(Leaf()) == "Leaf"
    assert projector.solver_name(Outer()) == "Outer/Mid/Leaf"
    assert projector.solver_name(None) is None


def _twin_case(A, cols, e, w):
    """(eta of the twin, eta of LAPACK's dense Cholesky, kappa_B, K) on diag(2^e) A."""
    S = nr.gram_pow2(A, e)
    nr.assert_26_bits(S.data)
    B, C = bd.split(nr.pow2_rows(A, e), cols)
    v, K = bd.twin(B, C, w)
    kappa_B = nr.scaled_cond(nr.gram_pow2(bd.split(A, cols)[0], e))
    return nr.backward_error(S, v, w), nr.backward_error(S, bd.lapack_dense(S, w), w), kappa_B, K


def test_twin_agrees_with_a_dense_solve_and_sets_c_twin():
    """The twin against LAPACK's dense Cholesky of the full S on every case of the GPU test, and
    C_TWIN: the largest eta / (kappa_B trace(K) u) the twin reaches there.  The dominant case's
    trace(K) lies between the two guards (the twin does not refine: its figures are printed)."""
    worst, worst_case, worst_eta = 0.0, None, 0.0
    for k in bd.SOLVE_K:
        for m, p, fill, graded in bd.solve_cases(k):
            A, cols, e, w = bd.build(k, m, p, fill, graded)
            assert len(cols) == p and A.shape[0] == m
            eta, lap, kappa_B, K = _twin_case(A, cols, e, w)
            # agreement with the dense solve, in the backward-error sense: both solve the same
            # system to within kappa_B kappa(K) of each other's error
            assert eta <= 64 * kappa_B * np.trace(K) * U, (k, m, p, eta / U)
            assert lap <= 64 * U, (k, m, p, lap / U)
            ratio = eta / (kappa_B * np.trace(K) * U)
            worst_eta = max(worst_eta, eta / U)
            if ratio > worst:
                worst, worst_case = ratio, (k, m, p, fill, graded, eta / U, kappa_B, np.trace(K))
    A, cols, e, w = bd.dominant_case()
    eta, lap, kappa_B, K = _twin_case(A, cols, e, w)
    from ipsolver.bordered import GROWTH_REFINE, GROWTH_MAX
    assert GROWTH_REFINE < np.trace(K) < GROWTH_MAX, np.trace(K)
    print("dominant: twin eta/u %.3g, LAPACK %.3g, kappa_B %.3g, trace(K) %.3g, kappa_2(K) %.3g"
          % (eta / U, lap / U, kappa_B, np.trace(K), np.linalg.cond(K)))
    print("largest twin eta/u %.3g; largest eta/(kappa_B trace(K) u) %.3g at %r"
          % (worst_eta, worst, worst_case))
    assert bd.C_TWIN >= worst, (worst, worst_case)


def test_other_inputs_of_the_gpu_test():
    from ipsolver.bordered import GROWTH_MAX
    A, cols = bd.huge_growth_case()
    B, C = bd.split(A, cols)
    _, K = bd.twin(B, C, np.ones(A.shape[0]))
    assert np.trace(K) > 4 * GROWTH_MAX, np.trace(K)
    assert _split(A, 64, 4) is not None and _split(A, 8, 4) is None
    A, cols = bd.identical_rows_case()
    B, C = bd.split(A, cols)
    SB = nr.gram_pow2(B).toarray()
    assert np.array_equal(SB[16], SB[17])                       # B B' exactly singular
    assert nr.scaled_cond(nr.gram_pow2(A)) < 1e8                # A A' is not
    s = _split(A, 64, 4)
    assert s is not None and np.array_equal(s.cols, cols) and 8 < s.k <= 16
    J, rhs, target = bd.staged_problem_with_parameters()
    s = _split(J, 64, 4)
    assert s is not None and s.p == 2 and s.k == 11
    assert _split(J, 8, 4) is None
