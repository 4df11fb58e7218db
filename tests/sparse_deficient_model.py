"""numpy model of the pivot-skipping Cholesky factorization (``PivotSkippingNestedSolver``,
ipsolver/nested.py) and of the operators built on it (``SparseDeficientProjector``,
ipsolver/sparse_deficient.py): what the library is compared with.  The elimination order is the
library's own nested-dissection order (``ipx_nd_order`` on the host, as
tests/test_nested_dissection_host.py calls it); the arithmetic is a plain dense right-looking
Cholesky of ``P A A' P'`` in fp64, slow on purpose.  No GPU.
"""
import numpy as np
import scipy.sparse as sps

RTOL = 2.0 ** -43                       # IPX_PIVOT_RTOL


def analysis(A, leaf):
    """The library's host analysis of the pattern of A (perm, sn_ptr, level, ...)."""
    from ipsolver import nested
    from ipsolver.banded import HostPattern
    A = sps.csr_matrix(A)
    return nested._NdSymbolic(HostPattern(A.indptr, A.indices, A.shape), leaf)


class SkippingCholesky:
    """``P S P' = L L'`` over the kept positions, S = A A' (dense).  ``skipped``: the positions
    whose pivot d met ``|d| <= 2^-43 S_kk``; ``dropped``: their rows, ascending; ``kept_ratio`` /
    ``dropped_ratio``: min d / S_kk over the kept, max |d| / S_kk over the skipped pivots (0 where
    S_kk = 0: a zero row).  ``keep_factor=False``: the ratios and the skipped positions only (the
    table of DESIGN.md section 4p at sizes whose dense L is not wanted)."""

    def __init__(self, A, perm, keep_factor=True):
        A = sps.csr_matrix(A)
        self.A = A
        self.perm = np.asarray(perm, dtype=np.int64)
        m = A.shape[0]
        S = np.asarray(A.dot(A.T).toarray())[np.ix_(self.perm, self.perm)]
        diag0 = np.diag(S).copy()
        L = np.zeros((m, m)) if keep_factor else None
        skipped = []
        kept_ratio, dropped_ratio = np.inf, 0.0
        for k in range(m):
            d = S[k, k]
            if abs(d) <= RTOL * diag0[k]:
                skipped.append(k)
                if diag0[k] > 0:
                    dropped_ratio = max(dropped_ratio, abs(d) / diag0[k])
                continue
            assert d > 0, "a negative pivot: not a model case"
            kept_ratio = min(kept_ratio, d / diag0[k])
            # (the rows with an entry in column k only: the others would subtract exact zeros)
            nz = k + 1 + np.flatnonzero(S[k + 1:, k])
            col = S[nz, k] / np.sqrt(d)
            S[np.ix_(nz, nz)] -= np.outer(col, col)
            if keep_factor:
                L[k, k] = np.sqrt(d)
                L[nz, k] = col
        self.L = L
        self.skipped = np.array(skipped, dtype=np.int64)
        self.dropped = np.sort(self.perm[self.skipped])
        self.kept = np.setdiff1d(np.arange(m), self.dropped)
        self.kept_ratio, self.dropped_ratio = kept_ratio, dropped_ratio
        self.rank = m - len(skipped)

    def solve(self, w):
        """K+ w: (A_S A_S')^-1 w_S on the kept rows, 0 on the dropped ones."""
        import scipy.linalg
        keep = np.setdiff1d(np.arange(len(self.perm)), self.skipped)
        Lk = self.L[np.ix_(keep, keep)]
        y = scipy.linalg.solve_triangular(Lk, np.asarray(w)[self.perm[keep]], lower=True)
        out = np.zeros(len(self.perm))
        out[self.perm[keep]] = scipy.linalg.solve_triangular(Lk.T, y, lower=False)
        return out

    # -- the operators of ipsolver/sparse_deficient.py, statement by statement
    def _woodbury(self):
        A, D = self.A, self.dropped
        Yw = np.column_stack([self.solve(A.dot(A[d].toarray().ravel())) for d in D]) \
            if len(D) else np.zeros((A.shape[0], 0))
        C = np.eye(len(D)) + Yw.T @ Yw
        return Yw, C

    def operators(self):
        """(Z, LS, Y) as functions of numpy vectors."""
        A, D, S = self.A, self.dropped, self.kept
        Yw, C = self._woodbury()

        def correct(u):
            return u - Yw @ np.linalg.solve(C, Yw.T @ u) if len(D) else u

        def null_space(x):
            return x - A.T.dot(self.solve(A.dot(x)))

        def least_squares(x):
            u = correct(self.solve(A.dot(x)))
            out = u.copy()
            out[D] = Yw.T @ u
            return out

        def row_space(b):
            t = np.zeros(len(b))
            t[S] = b[S] + (Yw @ b[D])[S]
            return A.T.dot(self.solve(correct(t)))
        return null_space, least_squares, row_space


def positions(sym, model):
    """Per skipped position (supernode, position inside its own rows, own rows s, tree level)."""
    out = []
    for k in model.skipped:
        j = int(np.searchsorted(sym.sn_ptr, k, side="right") - 1)
        out.append((j, int(k - sym.sn_ptr[j]), int(sym.sn_ptr[j + 1] - sym.sn_ptr[j]),
                    int(sym.level[j])))
    return out
