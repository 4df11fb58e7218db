"""Host side of the linked solver (ipsolver/linked.py): the pattern analysis, the inputs of
tests/test_gpu_link_rows.py and the numpy twin whose error sets C_TWIN_LINK.  No GPU."""
import numpy as np
import pytest
import scipy.sparse as sps

import blocktri_cases as bc
import link_cases as lc
import normal_ref as nr

U = nr.U


def _pattern(A):
    from ipsolver.bordered import HostPattern
    A = sps.csr_matrix(A)
    A.sort_indices()
    return HostPattern(A.indptr, A.indices, A.shape)


def _split(A, reach, limit, border=0):
    from ipsolver.linked import link_split
    return link_split(_pattern(A), reach, limit, border)


def _check_split(A, s, rows):
    """The index lists reproduce B and D exactly."""
    A = sps.csr_matrix(A)
    m, n = A.shape
    q = len(rows)
    B, D = lc.split(A, rows)
    assert np.array_equal(s.d_rows, rows) and s.q == q and s.m_b == m - q
    assert np.array_equal(np.sort(np.concatenate((s.b_rows, s.d_rows))), np.arange(m))
    got_B = sps.csr_matrix((A.data[s.b_src], s.host.indices_h, s.host.indptr_h), shape=B.shape)
    assert abs(got_B - B).nnz == 0
    Dt = np.zeros(n * q)
    Dt[s.c_dst] = A.data[s.c_src]
    assert len(np.unique(s.c_dst)) == len(s.c_dst)
    assert np.array_equal(Dt.reshape(n, q).T, D)                   # row-major n x q
    assert np.array_equal(s.dst_row[s.b_rows], np.arange(m - q))
    assert np.array_equal(s.dst_row[s.d_rows], m - q + np.arange(q))


@pytest.mark.parametrize("where", lc.WHERE)
def test_split_rows_reproduces_b_and_d(where):
    from ipsolver.linked import split_rows
    rng = np.random.default_rng(1)
    A, rows = lc.linked(rng, bc.band_rows(rng, 40, 4, lim=2 ** 4), 3, 0.3, 2 ** 4, where)
    s = split_rows(_pattern(A), rows)
    _check_split(A, s, rows)
    assert s.k == 4
    # rows that are no link rows at all are taken as given
    odd = np.array([1, 7, 20])
    _check_split(A, split_rows(_pattern(A), odd), odd)
    assert split_rows(_pattern(A), np.arange(A.shape[0])) is None      # no band row left


@pytest.mark.parametrize("fill", [1.0, 0.3])
@pytest.mark.parametrize("where", lc.WHERE)
@pytest.mark.parametrize("k,reach,q", [(1, 8, 1), (1, 8, 4), (1, 8, 32), (9, 64, 1), (9, 64, 4),
                                       (9, 64, 32)])
def test_link_split_finds_the_planted_rows(k, reach, q, where, fill):
    rng = np.random.default_rng([k, q, int(10 * fill)])
    mB = 4 * reach + 8
    A, rows = lc.linked(rng, bc.band_rows(rng, mB, k, lim=2 ** 4), q, fill, 2 ** 4, where)
    s = _split(A, reach, 32)
    assert s is not None
    # every planted row reaches rows further than `reach` away at these fills: exactly those
    _check_split(A, s, rows)
    B, _ = lc.split(A, s.d_rows)
    assert bc.half_bandwidth(B @ B.T) <= reach and s.k <= reach
    # one row short
    assert _split(A, reach, q - 1) is None
    assert _split(A, reach, q) is not None
    # a permutation of the columns changes nothing
    perm = rng.permutation(A.shape[1])
    sp = _split(sps.csr_matrix(sps.csc_matrix(A)[:, perm]), reach, 32)
    assert sp is not None and np.array_equal(sp.d_rows, rows)
    # cached on the pattern, per (reach, limit, border)
    from ipsolver.linked import link_split
    pat = _pattern(A)
    assert link_split(pat, reach, 32) is link_split(pat, reach, 32)


def test_link_split_returns_none():
    import bordered_cases as bd
    rng = np.random.default_rng(5)
    base = bc.band_rows(rng, 90, 4, lim=2 ** 4)
    assert _split(base, 8, 4) is None                                   # a plain band
    # too wide a band: thinning 600 rows from half bandwidth 9 to 8 takes more than 32 of them
    assert _split(bc.band_rows(rng, 600, 9, lim=2 ** 4), 8, 32) is None
    A, rows = lc.linked(rng, base, 2, 1.0, 2 ** 4)
    assert _split(A, 8, 0) is None and _split(A, 8, 1) is None
    assert _split(A, 8, 2) is not None
    # a dense column is a clique of m rows: refused at once while border columns are off,
    # left to the bordered solver of B when they are on
    C, cols = bd.bordered(rng, A, 1, 1.0, 2 ** 4)
    assert _split(C, 8, 4) is None
    s = _split(C, 8, 4, border=1)
    assert s is not None and np.array_equal(s.d_rows, rows)
    assert _split(bd.bordered(rng, A, 2, 1.0, 2 ** 4)[0], 8, 4, border=1) is None
    big = bc.band_rows(rng, 20000, 1, lim=2)
    C, _ = bd.bordered(rng, big, 1, 1.0, 2)
    import time
    t0 = time.perf_counter()
    assert _split(C, 8, 32) is None
    assert time.perf_counter() - t0 < 1.0                               # (no m^2 work)


def test_periodicity_block_gets_a_valid_cover():
    """x_N = x_0 on ocp_rows: d rows that couple the first stage with the last; any cover of at
    most d rows that leaves a band is right."""
    d, c, stages = 6, 2, 30
    rng = np.random.default_rng(9)
    J = bc.ocp_rows(d, c, stages, rng)
    per = sps.lil_matrix((d, J.shape[1]))
    for i in range(d):
        per[i, i], per[i, stages * (d + c) + i] = 1.0, -1.0
    A = sps.vstack((J, per.tocsr()), format="csr")
    s = _split(A, 64, 8)
    assert s is not None and 1 <= s.q <= d and s.m_b == A.shape[0] - s.q
    B, _ = lc.split(A, s.d_rows)
    assert bc.half_bandwidth(B @ B.T) <= 64 and s.k <= 64
    _check_split(A, s, s.d_rows)
    J, rhs, target, rows = lc.staged_problem_with_links()
    s = _split(J, 64, 8)
    assert s is not None and s.q <= len(rows) and rows[0] in s.d_rows     # (the budget row)
    B, _ = lc.split(J, s.d_rows)
    assert bc.half_bandwidth(B @ B.T) <= 64


def _twin_case(A, rows, e, w):
    """(eta of the twin, eta of LAPACK's dense Cholesky, kappa_B, K, F) on diag(2^e) A."""
    m = A.shape[0]
    S = nr.gram_pow2(A, e)
    nr.assert_26_bits(S.data)
    assert np.linalg.matrix_rank(sps.csr_matrix(A).toarray()) == m         # full row rank
    B, D = lc.split(nr.pow2_rows(A, e), rows)
    v, K, F = lc.twin(B, D, lc.band_first(rows, m, w))
    v = lc.caller_order(rows, m, v)
    keep = np.ones(m, dtype=bool)
    keep[rows] = False
    kappa_B = nr.scaled_cond(nr.gram_pow2(lc.split(A, rows)[0], e[keep]))
    return (nr.backward_error(S, v, w), nr.backward_error(S, lc.lapack_dense(S, w), w), kappa_B,
            K, F)


def test_twin_agrees_with_a_dense_solve_and_sets_c_twin_link():
    """The twin against LAPACK's dense Cholesky of the full S on every case of the GPU test, and
    C_TWIN_LINK: the largest eta / (kappa_B u) the twin reaches there."""
    worst, worst_case, worst_lap = 0.0, None, 0.0
    for k in lc.SOLVE_K:
        for mB, q, fill, graded, where in lc.solve_cases(k):
            A, rows, e, w = lc.build(k, mB, q, fill, graded, where)
            assert len(rows) == q and A.shape[0] == mB + q
            eta, lap, kappa_B, K, F = _twin_case(A, rows, e, w)
            ratio = eta / (kappa_B * U)
            print("k%d m_B%d q%d fill%.1f%s %s: twin eta/u %.3g, LAPACK dense %.3g, kappa_B %.3g, "
                  "max F_jj/K_jj %.3g" % (k, mB, q, fill, " graded" if graded else "", where,
                                          eta / U, lap / U, kappa_B, lc.cancellation(K, F)))
            worst_lap = max(worst_lap, lap / U)
            if ratio > worst:
                worst, worst_case = ratio, (k, mB, q, fill, graded, where, eta / U, kappa_B)
    print("largest twin eta/(kappa_B u) %.3g at %r; largest LAPACK dense eta/u %.3g"
          % (worst, worst_case, worst_lap))
    assert worst <= lc.C_TWIN_LINK <= 2 * worst, (worst, worst_case)


def test_nearly_dependent_link_rows_need_no_guard():
    """Link rows that are nearly combinations of band rows: the twin is no worse than 8 x LAPACK's
    dense Cholesky of the full S, whatever F_jj / K_jj."""
    A, rows, e, w = lc.nearly_dependent_case()
    eta, lap, kappa_B, K, F = _twin_case(A, rows, e, w)
    print("nearly dependent: twin eta/u %.3g, LAPACK dense %.3g, kappa_B %.3g, max F_jj/K_jj %.3g"
          % (eta / U, lap / U, kappa_B, lc.cancellation(K, F)))
    assert lc.cancellation(K, F) > 100
    assert eta <= 8 * lap
    assert eta <= 8 * lc.C_TWIN_LINK * kappa_B * U


def test_other_inputs_of_the_gpu_test():
    A, rows, e, w = lc.nearly_dependent_case(noise=False)
    B, D = lc.split(A, rows)
    assert len(rows) == 1
    assert np.linalg.matrix_rank(A.toarray()) == A.shape[0] - 1        # K exactly singular
    A, rows = lc.identical_link_rows_case()
    assert np.array_equal(A[rows[0]].toarray(), A[rows[1]].toarray())
    s = _split(A, 8, 4)
    assert s is not None and np.array_equal(s.d_rows, rows)
    A, rows = lc.identical_band_rows_case()
    B, _ = lc.split(A, rows)
    SB = nr.gram_pow2(B).toarray()
    assert np.array_equal(SB[16], SB[17])                               # B B' exactly singular
    s = _split(A, 64, 4)
    assert s is not None and np.array_equal(s.d_rows, rows)


def test_option_plumbing():
    from ipsolver import projector
    import ipsolver
    assert projector.link_rows_limit() == 0
    for bad in (-1, lc.Q_MAX + 1, 1.5, "4", True):
        with pytest.raises(ValueError, match="link_rows"):
            with projector.link_rows(bad):
                pass
    assert projector._hip.load().ipx_border_pmax() == lc.Q_MAX
    assert projector._hip.load().ipx_border_rows_per_group() == lc.ROWS_PER_GROUP
    with pytest.raises(RuntimeError):
        with projector.link_rows(4):
            assert projector.link_rows_limit() == 4
            with projector.link_rows(0):
                assert projector.link_rows_limit() == 0
            assert projector.link_rows_limit() == 4
            raise RuntimeError("inside")
    assert projector.link_rows_limit() == 0
    with projector.link_rows(32):
        assert projector.link_rows_limit() == 32
    assert projector.link_rows_limit() == 0
    calls = []
    with pytest.raises(ValueError, match="link_rows"):
        ipsolver.minimize_constrained(lambda x: calls.append(1) or 0.0, np.zeros(2),
                                      lambda x: np.zeros(2), options={"link_rows": 33})
    assert not calls
