"""Rank-deficient dense Jacobians for the tests of ``rank_deficient = "pivoted-qr"``
(ipsolver/dense_cod.py): builders shared by tests/test_rank_deficient_host.py,
tests/test_gpu_rank_deficient.py, tests/test_gpu_rank_deficient_e2e.py and the fixture's
generator tests/golden/make_golden_rank_deficient.py.

Every matrix is scaled by 2^-10 (exact): the singular values that are zero in exact arithmetic --
a few eps ||A||_2 as LAPACK computes them -- then lie below the oracle's absolute tol = 1e-15, so
that the oracle's SVD exit and the device's relative rule drop the same ones (the scaling of
tests/test_gpu_dense_qr.py::test_rank_deficient_keeps_the_svd_exit).
"""
import numpy as np
import scipy.linalg

import dense_qr_cases

SCALE = 2.0 ** -10
ORACLE_TOL = 1e-15

# one panel exactly; panel + 1; two panels + 2 with a ragged n; four panels
SHAPES = [(64, 64), (65, 300), (130, 700), (200, 1000)]
ROW_KINDS = ("duplicate", "combination", "zero")
GRADED = [(130, 700, 5), (200, 1000, 70)]
GRADED_CONDS = (1e3, 1e6, 1e8)


def row_replaced(kind, m, n):
    """Row m - 3 of a Gaussian matrix replaced: rank m - 1."""
    rng = np.random.default_rng(7 * m + len(kind))
    A = rng.standard_normal((m, n)) * SCALE
    r = m - 3
    if kind == "duplicate":
        A[r] = A[5]
    elif kind == "combination":
        A[r] = rng.standard_normal(r) @ A[:r]
    else:
        assert kind == "zero"
        A[r] = 0.0
    return A, m - 1


def lowrank(m, n):
    """B C / sqrt(r) of rank r = max(1, m // 2)."""
    rng = np.random.default_rng(1000 * m + n)
    r = max(1, m // 2)
    A = rng.standard_normal((m, r)) @ rng.standard_normal((r, n)) / np.sqrt(r) * SCALE
    return A, r


def zeros_all(m, n):
    return np.zeros((m, n)), 0


def graded(m, n, k, cond):
    """A rank m - k matrix with the singular values logspace(0, -log10 cond, m - k), k more rows
    that are combinations of its rows, the rows permuted."""
    rng = np.random.default_rng(1000 * m + n + int(np.log10(cond)))
    r = m - k
    U, _ = np.linalg.qr(rng.standard_normal((r, r)))
    V, _ = np.linalg.qr(rng.standard_normal((n, r)))
    B = (U * np.logspace(0, -np.log10(cond), r)) @ V.T
    C = rng.standard_normal((k, r)) / np.sqrt(r)
    A = np.vstack([B, C @ B])[rng.permutation(m)] * SCALE
    return A, r


def all_cases():
    """(name, builder arguments) of every case; ``build(*args)`` makes it."""
    out = [("lowrank-3x5", ("lowrank", 3, 5)), ("zeros-all-3x5", ("zeros-all", 3, 5))]
    for m, n in SHAPES:
        for kind in ROW_KINDS + ("lowrank", "zeros-all"):
            out.append(("%s-%dx%d" % (kind, m, n), (kind, m, n)))
    for m, n, k in GRADED:
        for cond in GRADED_CONDS:
            out.append(("graded-%dx%d-k%d-%.0e" % (m, n, k, cond), ("graded", m, n, k, cond)))
    return out


def build(kind, m, n, k=None, cond=None):
    """(A, intended rank)"""
    if kind in ROW_KINDS:
        return row_replaced(kind, m, n)
    if kind == "lowrank":
        return lowrank(m, n)
    if kind == "zeros-all":
        return zeros_all(m, n)
    assert kind == "graded"
    return graded(m, n, k, cond)


def oracle_rank(A):
    """The rank the oracle works with: its QR test must send A to the SVD exit
    (oracle/projections.py:124), which keeps the singular values > tol."""
    R = scipy.linalg.qr(A.T, pivoting=True, mode="r")[0]
    assert np.linalg.norm(R[A.shape[0] - 1, :], np.inf) < ORACLE_TOL
    return int(np.count_nonzero(scipy.linalg.svd(A, compute_uv=False) > ORACLE_TOL))


def kept_condition(A, rank):
    """sigma_1 / sigma_rank of A (1 for rank 0)."""
    if rank == 0:
        return 1.0
    s = scipy.linalg.svd(A, compute_uv=False)
    return float(s[0] / s[rank - 1])


# ---- the end-to-end problem: dense_qr_cases.problem(cond) scaled by 2^-10, six consistent
# combination rows added, the rows permuted
E2E_CONDS = (1e3, 1e6)
E2E_EXTRA = 6


def e2e_problem(cond):
    """(A, H, c, b, independent): A is (m + 6) x n of rank m; ``A[independent]``,
    ``b[independent]`` are the m rows of the full-rank problem (for ``kkt_point``)."""
    A0, H, c, b0 = dense_qr_cases.problem(cond)
    A0, b0 = A0 * SCALE, b0 * SCALE
    m = A0.shape[0]
    rng = np.random.default_rng(100 + int(np.log10(cond)))
    C = rng.standard_normal((E2E_EXTRA, m)) / np.sqrt(m)
    order = rng.permutation(m + E2E_EXTRA)
    A = np.vstack([A0, C @ A0])[order]
    b = np.concatenate([b0, C @ b0])[order]
    independent = np.argsort(order)[:m]
    return A, H, c, b, independent
