"""The exact residual and the scaled backward error of tests/normal_ref.py (what
tests/test_gpu_normal_solve.py judges every solve with S = A A' by) against rational
arithmetic (fractions.Fraction).  No GPU."""
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sps

import normal_ref as nr


def _band_int(rng, m, k, lim=2 ** 10):
    """Integer rows over columns 3i .. 3i + 3k: A A' of half bandwidth k."""
    w = 3 * k + 1
    cols = (3 * np.arange(m)[:, None] + np.arange(w)[None, :]).ravel()
    return sps.csr_matrix((nr.int_values(rng, m * w, lim), cols, np.arange(0, m * w + 1, w)),
                          shape=(m, 3 * m + 3 * k + 1))


def _wide_vector(rng, m, spread):
    """Normal values times 2^e, e uniform in [-spread, spread] (far from the subnormals)."""
    return rng.standard_normal(m) * np.ldexp(1.0, rng.integers(-spread, spread + 1, m))


def _frac_residual(S, v, w):
    S = sps.csr_matrix(S)
    out = []
    for i in range(S.shape[0]):
        acc = Fraction(w[i])
        for p in range(S.indptr[i], S.indptr[i + 1]):
            acc -= Fraction(S.data[p]) * Fraction(v[S.indices[p]])
        out.append(acc)
    return out


def _frac_eta(S, v, w):
    S = sps.csr_matrix(S)
    f = nr.pow2_scale(S)
    r = _frac_residual(S, v, w)
    two = [Fraction(2) ** int(x) for x in f]
    num = max(abs(r[i]) / two[i] for i in range(len(r)))
    normS = max(sum(abs(Fraction(S.data[p])) / (two[i] * two[S.indices[p]])
                    for p in range(S.indptr[i], S.indptr[i + 1])) for i in range(S.shape[0]))
    dv = max(abs(Fraction(v[i])) * two[i] for i in range(len(v)))
    dw = max(abs(Fraction(w[i])) / two[i] for i in range(len(w)))
    return num / (normS * dv + dw)


@pytest.mark.parametrize("graded", [False, True])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("seed", range(3))
def test_gram_pow2_is_the_exact_product(graded, k, seed):
    """S from the integer product times 2^(e_i + e_j) equals A A' of the scaled rows in
    rational arithmetic, entry by entry."""
    rng = np.random.default_rng(seed)
    m = 9
    A_int = _band_int(rng, m, k)
    e = rng.integers(-30, 31, m) if graded else np.zeros(m, np.int64)
    S = nr.gram_pow2(A_int, e).toarray()
    A = nr.pow2_rows(A_int, e).toarray()
    for i in range(m):
        for j in range(m):
            want = sum(Fraction(A[i, t]) * Fraction(A[j, t]) for t in range(A.shape[1]))
            assert Fraction(S[i, j]) == want, (i, j)


@pytest.mark.parametrize("graded", [False, True])
@pytest.mark.parametrize("k", [1, 2, 5])
@pytest.mark.parametrize("seed", range(3))
def test_residual_exact_is_correctly_rounded(graded, k, seed):
    """residual_exact against Fraction, rounded once: bit for bit -- for v whose entries span
    2^-300 .. 2^300 and for w = fl(S v) (+ a last-bit nudge), where r is all cancellation."""
    rng = np.random.default_rng(100 + seed)
    m = 14
    A_int = _band_int(rng, m, k)
    e = rng.integers(-30, 31, m) if graded else np.zeros(m, np.int64)
    S = nr.gram_pow2(A_int, e)
    for v, w in ((_wide_vector(rng, m, 300), _wide_vector(rng, m, 40)),
                 (_wide_vector(rng, m, 20), None)):
        if w is None:
            w = S @ v
            w[::3] = np.nextafter(w[::3], np.inf)
        got = nr.residual_exact(S, v, w)
        want = np.array([float(x) for x in _frac_residual(S, v, w)])
        assert np.array_equal(got, want), np.flatnonzero(got != want)


def test_residual_exact_refuses_entries_wider_than_26_bits():
    S = sps.csr_matrix(np.array([[2.0 ** 26 + 1.0]]))
    with pytest.raises(AssertionError):
        nr.residual_exact(S, np.ones(1), np.ones(1))
    nr.residual_exact(sps.csr_matrix(np.array([[(2.0 ** 26 - 1.0) * 2.0 ** 40]])), np.ones(1),
                      np.ones(1))


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("seed", range(3))
def test_backward_error_against_fractions_and_under_row_scaling(k, seed):
    """backward_error against the same formula in rational arithmetic (to rounding of the
    host's few float operations), and invariant under row scaling by powers of two: rows
    scaled by 2^e, w by 2^e, v by 2^-e give the SAME scaled system, hence the same value."""
    rng = np.random.default_rng(200 + seed)
    m = 12
    A_int = _band_int(rng, m, k)
    S0 = nr.gram_pow2(A_int)
    v = _wide_vector(rng, m, 30)
    w = S0 @ v + _wide_vector(rng, m, 2) * 1e-9
    eta0 = nr.backward_error(S0, v, w)
    want = float(_frac_eta(S0, v, w))
    assert eta0 > 0 and abs(eta0 - want) <= 1e-13 * want
    e = rng.integers(-30, 31, m)
    S1 = nr.gram_pow2(A_int, e)
    v1, w1 = np.ldexp(v, -e), np.ldexp(w, e)
    assert nr.backward_error(S1, v1, w1) == eta0
    assert abs(float(_frac_eta(S1, v1, w1)) - want) <= 1e-15 * want
    # a wrong solution has a large backward error; a solve of the scaled system (backward
    # stable there) a small one
    assert nr.backward_error(S1, 2 * v1, w1) > 0.1
    f = nr.pow2_scale(S1)
    x = np.ldexp(np.linalg.solve(nr.scaled_matrix(S1).toarray(), np.ldexp(w1, -f)), -f)
    assert nr.backward_error(S1, x, w1) <= 100 * m * nr.U


def test_scaled_cond_ignores_row_scaling():
    rng = np.random.default_rng(7)
    A_int = _band_int(rng, 30, 2)
    c0 = nr.scaled_cond(nr.gram_pow2(A_int))
    c1 = nr.scaled_cond(nr.gram_pow2(A_int, rng.integers(-30, 31, 30)))
    assert abs(c0 - c1) <= 1e-8 * c0
