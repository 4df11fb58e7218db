"""Shared by the constraint quasi-Newton tests: Jacobian patterns, their transposes, a numpy
restatement of ``ipx_csr_tdiff_dot`` and a caller of the library's host twin."""
import ctypes

import numpy as np
import scipy.sparse as sps


def _pattern(rows, cols, m, n):
    M = sps.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(m, n))
    M.sum_duplicates()
    M.sort_indices()
    return M.indptr.astype(np.int32), M.indices.astype(np.int32), (m, n)


def tridiagonal():
    m, n = 5, 7
    ij = [(i, j) for i in range(m) for j in range(n) if abs(i - j) <= 1]
    return _pattern([i for i, _ in ij], [j for _, j in ij], m, n)


def empty_row_and_column():
    """row 2 and column 3 hold nothing"""
    m, n = 6, 9
    ij = [(0, 0), (0, 4), (1, 1), (1, 2), (1, 8), (3, 0), (3, 5), (4, 4), (4, 6), (4, 7), (5, 8)]
    return _pattern([i for i, _ in ij], [j for _, j in ij], m, n)


def arrow():
    """column 0 full: row 0 of the transpose has 2100 > IPX_SPMV_TILE_NNZ = 2048 entries"""
    m, n = 2100, 300
    rows = list(range(m)) + [i for i in range(m) if i % n]
    cols = [0] * m + [i % n for i in range(m) if i % n]
    return _pattern(rows, cols, m, n)


def one_variable():
    return _pattern([0, 2], [0, 0], 3, 1)


PATTERNS = [("tridiagonal", tridiagonal), ("empty", empty_row_and_column), ("arrow", arrow),
            ("n1", one_variable)]


def transpose(indptr, indices, shape):
    """(t_indptr, t_indices, perm) with valT = val[perm], as ``CSRPattern.transpose`` builds it"""
    m, n = shape
    nnz = len(indices)
    tag = sps.csr_matrix((np.arange(1, nnz + 1, dtype=np.float64), indices, indptr), shape=(m, n))
    t = sps.csr_matrix(tag.T)
    t.sort_indices()
    return (t.indptr.astype(np.int32), t.indices.astype(np.int32),
            (t.data - 1).astype(np.int64))


def operands(shape, nnz, seed):
    rng = np.random.default_rng(seed)
    m, n = shape
    return dict(val_new=rng.standard_normal(nnz), val_old=rng.standard_normal(nnz),
                v=rng.standard_normal(m), base_new=rng.standard_normal(n),
                base_old=rng.standard_normal(n), y0=rng.standard_normal(n))


def restatement(t_indptr, t_indices, perm, val_new, val_old, v, base_new, base_old, y0,
                accumulate):
    """the entry's definition, the same loop order with plain *, -, +"""
    n = len(t_indptr) - 1
    y = np.empty(n)
    for j in range(n):
        head = y0[j] if accumulate else 0.0
        base = base_new[j] - base_old[j] if base_new is not None else 0.0
        s = 0.0
        for k in range(t_indptr[j], t_indptr[j + 1]):
            s = s + v[t_indices[k]] * (val_new[perm[k]] - val_old[perm[k]])
        y[j] = (head + base) + s
    return y


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_twin(lib, shape, t_indptr, t_indices, perm, val_new, val_old, v, base_new, base_old, y0,
              accumulate):
    m, n = shape
    c = lambda a, t=np.float64: None if a is None else np.ascontiguousarray(a, dtype=t)
    y = np.array(y0, dtype=float, copy=True) if accumulate else np.full(n, np.nan)
    arrs = [c(t_indptr, np.int32), c(t_indices, np.int32), c(perm, np.int64), c(val_new),
            c(val_old), c(v), c(base_new), c(base_old)]
    rc = lib.ipx_csr_tdiff_dot_host(n, m, len(t_indices), *[_ptr(a) for a in arrs], _ptr(y),
                                    1 if accumulate else 0)
    assert rc == 0, rc
    return y
