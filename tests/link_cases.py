"""Matrix generators, the host twin and the case list of tests/test_gpu_link_rows.py (no GPU
needed here).

A case is a band B (``blocktri_cases.band_rows`` / ``ocp_rows``) with q integer link rows D put
among its rows: ``S = A A' = [S_B E; E' F]``.  Every link row also has one column of its own
holding a non-zero integer (the slack of a linking inequality), so every case has full row rank
whatever m_B and q.  Every value is an integer small enough that every entry of S keeps within 26
significant bits, so ``normal_ref.gram_pow2``, ``residual_exact`` and ``backward_error`` apply
unchanged (also with rows scaled by powers of two).
"""
import numpy as np
import scipy.linalg
import scipy.sparse as sps

import blocktri_cases as bc
import normal_ref as nr

ROWS_PER_GROUP = 256                    # ipx_border_rows_per_group() (both tests check it)
Q_MAX = 32                              # ipx_border_pmax()
R = ROWS_PER_GROUP
SOLVE_MB = (1, 2, R - 1, R, R + 1, 2 * R + 1)
SOLVE_Q = (1, 2, 31, 32)
SOLVE_K = (1, 4, 9, 17)                 # inner: banded (1, 4), block tridiagonal (9, 17)
WHERE = ("top", "middle", "bottom")
LIM_BAND, LIM_D = 2 ** 7, 2 ** 7        # entries of F stay below 2^26 up to n ~ 4000

# The largest eta / (kappa_B u) the host twin (LAPACK) reaches over ``solve_cases()``:
# tests/test_link_rows_host.py computes it (0.708: k = 4, m_B = 1, q = 2, bottom, fill 0.3,
# graded, eta = 0.708 u with kappa_B = 1; from m_B = 255 on it stays below 0.04; LAPACK's dense
# Cholesky of the full S gives the same eta within a factor of 4) and asserts that this constant
# is not below it and not more than twice it.
C_TWIN_LINK = 0.75


def linked(rng, base, q, fill, lim, where="bottom", private=True):
    """``base`` with q integer rows (|entry| <= lim, each column present with probability
    ``fill``, at least one entry per row) inserted above its rows ("top"), in the middle, or
    below them ("bottom"); ``private``: each new row also has a non-zero integer on a new column
    of its own (appended).  Returns (A, indices of the new rows)."""
    base = sps.csr_matrix(base)
    m, n = base.shape
    mask = rng.random((q, n)) < fill
    mask[np.arange(q), rng.integers(0, n, q)] = True
    D = np.where(mask, nr.int_values(rng, q * n, lim).reshape(q, n), 0.0)
    if private:
        D = np.hstack((D, np.diag(nr.int_values(rng, q, lim))))
        base = sps.hstack((base, sps.csr_matrix((m, q))), format="csr")
    at = {"top": 0, "middle": m // 2, "bottom": m}[where]
    A = sps.vstack((base[:at], sps.csr_matrix(D), base[at:]), format="csr")
    A.sort_indices()
    return A, at + np.arange(q)


def split(A, rows):
    """(B, D) of A: B the other rows (CSR, in order), D the rows ``rows`` (dense q x n)."""
    A = sps.csr_matrix(A)
    keep = np.ones(A.shape[0], dtype=bool)
    keep[rows] = False
    return sps.csr_matrix(A[np.flatnonzero(keep)]), A[rows].toarray()


def band_first(rows, m, x):
    """x (one entry per row of A, the caller's order) with the band rows first, then the link
    rows: the order of ``twin``."""
    keep = np.ones(m, dtype=bool)
    keep[rows] = False
    return np.concatenate((np.asarray(x)[keep], np.asarray(x)[rows]))


def caller_order(rows, m, x):
    """The inverse of ``band_first``."""
    keep = np.ones(m, dtype=bool)
    keep[rows] = False
    out = np.empty(m)
    out[keep], out[rows] = x[:m - len(rows)], x[m - len(rows):]
    return out


def twin(B, D, w):
    """The device's formula in numpy with LAPACK's Cholesky; w and v with the band rows first:
    (v, K, F).  Y = S_B^-1 E, K = F - E' Y, u = S_B^-1 w_B, K z = w_D - Y' w_B, v = (u - Y z, z)."""
    B = sps.csr_matrix(B)
    mB = B.shape[0]
    E, F = B @ D.T, D @ D.T
    fac = scipy.linalg.cho_factor((B @ B.T).toarray(), lower=True)
    u = scipy.linalg.cho_solve(fac, w[:mB])
    Y = scipy.linalg.cho_solve(fac, E)
    K = F - E.T @ Y
    z = scipy.linalg.cho_solve(scipy.linalg.cho_factor(K, lower=True), w[mB:] - Y.T @ w[:mB])
    return np.concatenate((u - Y @ z, z)), K, F


def lapack_dense(S, w):
    """LAPACK's dense Cholesky of the full S: the yardstick."""
    return scipy.linalg.cho_solve(scipy.linalg.cho_factor(sps.csr_matrix(S).toarray(), lower=True), w)


def cancellation(K, F):
    """max_j F_jj / K_jj: what the solver reports as ``cancellation``."""
    return float(np.max(np.diag(F) / np.diag(K)))


# ---------------------------------------------------------------------------- the case list
def solve_cases(k):
    """(m_B, q, fill, graded, where) of the solve test for inner half bandwidth k: every m_B with
    every q; fill (1.0 / 0.3) and grading alternate so that every q meets both fills and both
    gradings at the sizes around the partial-count boundaries; the place of the link rows goes
    round top, middle, bottom."""
    out = []
    ik = SOLVE_K.index(k)
    for im, mB in enumerate(SOLVE_MB):
        for iq, q in enumerate(SOLVE_Q):
            fill = 1.0 if (im + iq) % 2 == 0 else 0.3
            graded = ((im + iq) // 2 + ik) % 2 == 1
            out.append((mB, q, fill, graded, WHERE[(im + iq + ik) % 3]))
    return out


def _finish(rng, A, rows, graded):
    m = A.shape[0]
    e = rng.integers(-30, 31, m) if graded else np.zeros(m, np.int64)
    spread = 30 if graded else 4
    w = rng.standard_normal(m) * np.ldexp(1.0, rng.integers(-spread, spread + 1, m))
    return A, rows, e, w


def build(k, mB, q, fill, graded, where):
    """(A_int, link rows, e, w) of a solve case, seeded by the case alone; w in A's row order."""
    rng = np.random.default_rng([k, mB, q, int(10 * fill), int(graded), WHERE.index(where)])
    A, rows = linked(rng, bc.band_rows(rng, mB, k, lim=LIM_BAND), q, fill, LIM_D, where)
    return _finish(rng, A, rows, graded)


NEARLY = (9, 2 * R + 1, 32)             # (k, m_B, q)


def nearly_dependent_case(noise=True):
    """Link rows that are an integer combination of three band rows each (coefficients +-1, +-2;
    band entries <= 8) plus, with ``noise``, +-1 on two columns and 1 on a column of their own:
    F_jj / K_jj in the hundreds to thousands.  Without ``noise`` (one link row, no column of
    its own): K exactly singular."""
    k, mB, q = NEARLY
    rng = np.random.default_rng([81, k, mB, q, int(noise)])
    base = bc.band_rows(rng, mB, k, lim=2 ** 3)
    if not noise:
        q = 1
    n = base.shape[1]
    comb = np.zeros((q, mB))
    for j in range(q):
        comb[j, rng.choice(mB, 3, replace=False)] = rng.choice((-2, -1, 1, 2), 3)
    D = comb @ base.toarray()
    if noise:
        for j in range(q):
            D[j, rng.choice(n, 2, replace=False)] += rng.choice((-1, 1), 2)
        D = np.hstack((D, np.eye(q)))
        base = sps.hstack((base, sps.csr_matrix((mB, q))), format="csr")
    at = mB // 2
    A = sps.vstack((base[:at], sps.csr_matrix(D), base[at:]), format="csr")
    A.sort_indices()
    A.eliminate_zeros()
    return _finish(rng, A, at + np.arange(q), False)


def identical_link_rows_case(mB=80, k=4):
    """Two identical link rows below a band: K is exactly singular."""
    rng = np.random.default_rng([82, mB, k])
    A, rows = linked(rng, bc.band_rows(rng, mB, k, lim=2 ** 4), 1, 1.0, 2 ** 4, "bottom",
                     private=False)
    A = sps.vstack((A, A[rows]), format="csr")
    A.sort_indices()
    return A, np.array([mB, mB + 1])


def identical_band_rows_case(mB=80):
    """``bc.identical_rows`` (B B' exactly singular) plus one full link row."""
    rng = np.random.default_rng(5)
    A, rows = linked(rng, bc.identical_rows(rng, m=mB, k=9, at=16), 1, 1.0, 2 ** 4, "top")
    return A, rows


def staged_problem_with_links(seed=0, inequality=False):
    """``bc.staged_problem`` (d = 6, c = 2, 30 stages) with a budget row over every variable and
    a periodicity block x_N = x_0 (d rows): (J, rhs, target, link rows).  ``inequality``: the
    budget row is returned apart, as (J, rhs, target, link rows of J, budget row, its bound)."""
    J, _, _ = bc.staged_problem(seed=seed)
    d, c, stages = 6, 2, 30
    n = J.shape[1]
    rng = np.random.default_rng([seed, 83])
    budget = sps.csr_matrix(rng.uniform(0.25, 1.0, (1, n)))
    per = sps.lil_matrix((d, n))
    for i in range(d):
        per[i, i], per[i, stages * (d + c) + i] = 1.0, -1.0
    x_feas, target = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    m0 = J.shape[0]
    if inequality:
        Jp = sps.vstack((J, per.tocsr()), format="csr")
        Jp.sort_indices()
        return (Jp, Jp @ x_feas, target, m0 + np.arange(d), budget,
                float((budget @ x_feas)[0]) + 1.0)
    Jl = sps.vstack((J, budget, per.tocsr()), format="csr")
    Jl.sort_indices()
    return Jl, Jl @ x_feas, target, m0 + np.arange(1 + d)
