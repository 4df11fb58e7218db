"""Matrix generators, the host twin and the case list of tests/test_gpu_bordered.py (no GPU
needed here).

A case is a band B (``blocktri_cases.band_rows`` / ``ocp_rows``) with p integer columns C appended:
``A = [B | C]``, ``S = A A' = B B' + C C'``.  Every value is an integer small enough that every
entry of S keeps within 26 significant bits, so ``normal_ref.gram_pow2``, ``residual_exact`` and
``backward_error`` apply unchanged (also with rows scaled by powers of two).
"""
import numpy as np
import scipy.linalg
import scipy.sparse as sps

import blocktri_cases as bc
import normal_ref as nr

ROWS_PER_GROUP = 256                    # ipx_border_rows_per_group() (both tests check it)
P_MAX = 32                              # ipx_border_pmax()
R = ROWS_PER_GROUP
SOLVE_M = (1, 2, R - 1, R, R + 1, 2 * R + 1)
SOLVE_P = (1, 2, 31, 32)
SOLVE_K = (1, 4, 9, 17)                 # inner: banded (1, 4), block tridiagonal (9, 17)
LIM_BAND, LIM_C = 2 ** 7, 2 ** 7        # columns of the band's magnitude
LIM_BAND_DOM, LIM_C_DOM = 2 ** 4, 2 ** 10       # dominant columns: 64 x the band

# The largest eta / (kappa_B trace(K) u) the host twin (LAPACK) reaches over ``solve_cases()``:
# tests/test_bordered_host.py computes it (0.868: k = 4, m = 1, p = 1, eta = 0.97 u with
# kappa_B = 1 and trace(K) = 1.12; from m = 255 on it stays below 0.01) and asserts that this
# constant is not below it.
C_TWIN = 0.875


def bordered(rng, base, p, fill, lim_c, where="last"):
    """``base`` with p integer columns (|entry| <= lim_c, each row present with probability
    ``fill``, at least one entry per column) inserted before its columns ("first"), in the
    middle, or after them ("last").  Returns (A, indices of the new columns)."""
    base = sps.csr_matrix(base)
    m, n = base.shape
    mask = rng.random((m, p)) < fill
    mask[rng.integers(0, m, p), np.arange(p)] = True
    C = sps.csr_matrix(np.where(mask, nr.int_values(rng, m * p, lim_c).reshape(m, p), 0.0))
    at = {"first": 0, "middle": n // 2, "last": n}[where]
    A = sps.hstack((base[:, :at], C, base[:, at:]), format="csr")
    A.sort_indices()
    return A, at + np.arange(p)


def split(A, cols):
    """(B, C) of A = [B | C]: B with the columns ``cols`` emptied (CSR), C dense m x p."""
    A = sps.csr_matrix(A)
    keep = np.ones(A.shape[1], dtype=bool)
    keep[cols] = False
    B = A @ sps.diags(keep.astype(np.float64))
    B.eliminate_zeros()
    return sps.csr_matrix(B), A[:, cols].toarray()


def twin(B, C, w):
    """The device's formula in numpy with LAPACK's Cholesky: (v, K).
    v = u - Y K^-1 Y' w, u = S_B^-1 w, Y = S_B^-1 C, K = I + C' Y."""
    B = sps.csr_matrix(B)
    fac = scipy.linalg.cho_factor((B @ B.T).toarray(), lower=True)
    u = scipy.linalg.cho_solve(fac, w)
    Y = scipy.linalg.cho_solve(fac, C)
    K = np.eye(C.shape[1]) + C.T @ Y
    z = scipy.linalg.cho_solve(scipy.linalg.cho_factor(K, lower=True), Y.T @ w)
    return u - Y @ z, K


def lapack_dense(S, w):
    """LAPACK's dense Cholesky of the full S: the yardstick."""
    return scipy.linalg.cho_solve(scipy.linalg.cho_factor(sps.csr_matrix(S).toarray(), lower=True), w)


# ---------------------------------------------------------------------------- the case list
def solve_cases(k):
    """(m, p, fill, graded) of the solve test for inner half bandwidth k: every m with every p;
    fill (1.0 / 0.3) and grading alternate so that every p meets both fills and both gradings
    at the sizes around the partial-count boundaries."""
    out = []
    ik = SOLVE_K.index(k)
    for im, m in enumerate(SOLVE_M):
        for ip, p in enumerate(SOLVE_P):
            fill = 1.0 if (im + ip) % 2 == 0 else 0.3
            graded = ((im + ip) // 2 + ik) % 2 == 1
            out.append((m, p, fill, graded))
    return out


def _finish(rng, A, cols, graded):
    m = A.shape[0]
    e = rng.integers(-30, 31, m) if graded else np.zeros(m, np.int64)
    spread = 30 if graded else 4
    w = rng.standard_normal(m) * np.ldexp(1.0, rng.integers(-spread, spread + 1, m))
    return A, cols, e, w


def build(k, m, p, fill, graded):
    """(A_int, border columns, e, w) of a solve case, seeded by the case alone."""
    rng = np.random.default_rng([k, m, p, int(10 * fill), int(graded)])
    A, cols = bordered(rng, bc.band_rows(rng, m, k, lim=LIM_BAND), p, fill, LIM_C)
    return _finish(rng, A, cols, graded)


DOMINANT = (9, 2 * R + 1, 32)           # (k, m, p)


def dominant_case():
    """|C| up to 64 x the band's entries, p = 32: trace(K) past GROWTH_REFINE."""
    k, m, p = DOMINANT
    rng = np.random.default_rng([77, k, m, p])
    A, cols = bordered(rng, bc.band_rows(rng, m, k, lim=LIM_BAND_DOM), p, 1.0, LIM_C_DOM)
    return _finish(rng, A, cols, False)


def huge_growth_case(m=160, k=9, p=4):
    """A band with entries of magnitude <= 2 and integer columns in [2^12, 2^13): trace(K) past
    GROWTH_MAX = 2^26 (tests/test_bordered_host.py checks it on the twin)."""
    rng = np.random.default_rng([78, m, k, p])
    base = bc.band_rows(rng, m, k, lim=2)
    C = rng.integers(2 ** 12, 2 ** 13, (m, p)).astype(np.float64)
    A = sps.hstack((base, sps.csr_matrix(C)), format="csr")
    A.sort_indices()
    return A, base.shape[1] + np.arange(p)


def identical_rows_case(m=80):
    """``bc.identical_rows`` (B B' exactly singular) plus one full column that tells the two
    rows apart: A A' is positive definite, B B' is not."""
    rng = np.random.default_rng(4)
    base = bc.identical_rows(rng, m=m, k=9, at=16)
    c = nr.int_values(rng, m, 2 ** 4)
    c[16], c[17] = 5.0, -7.0
    A = sps.hstack((base, sps.csr_matrix(c[:, None])), format="csr")
    A.sort_indices()
    return A, np.array([base.shape[1]])


def border_only_row_case(m=80, k=9):
    """Row 30 has entries in the dense column only."""
    rng = np.random.default_rng([79, m, k])
    base = bc.band_rows(rng, m, k, lim=2 ** 4).tolil()
    base.rows[30], base.data[30] = [], []
    A, cols = bordered(rng, base.tocsr(), 1, 1.0, 2 ** 4)
    return A, cols


def staged_problem_with_parameters(npar=2, seed=0):
    """``bc.staged_problem`` with ``npar`` global parameter columns appended to J (entries of
    the band's magnitude): (J, rhs, target)."""
    J, _, _ = bc.staged_problem(seed=seed)
    rng = np.random.default_rng([seed, npar])
    J = sps.hstack((J, sps.csr_matrix(rng.uniform(-1, 1, (J.shape[0], npar)))), format="csr")
    J.sort_indices()
    n = J.shape[1]
    x_feas, target = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    return J, J @ x_feas, target
