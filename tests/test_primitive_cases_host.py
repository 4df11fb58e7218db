"""The integer-valued cases of tests/primitive_cases.py are what they claim to be: for every
output the sum of |terms| is below 2^53, so the float64 sum in forward order, in reversed
order and the int64 sum agree -- any summation order gives the int64 result -- and the
longdouble reference the real-valued cases are judged by reproduces the int64 one.  No GPU."""
import numpy as np
import pytest
import scipy.sparse as sps

import primitive_cases as pc

LD = np.longdouble


def check_terms(T):
    """T: (outputs, nterms) int64."""
    T = np.asarray(T, dtype=np.int64).reshape(len(T), -1)
    want = T.sum(axis=1)
    assert np.abs(T).sum(axis=1).max(initial=0) < pc.TWO53
    if T.shape[1] == 0:
        assert not want.any()
        return
    Tf = T.astype(np.float64)
    assert np.array_equal(np.cumsum(Tf, axis=1)[:, -1], want)              # forward, sequential
    assert np.array_equal(np.cumsum(Tf[:, ::-1], axis=1)[:, -1], want)     # reversed
    assert np.array_equal(T.astype(LD).sum(axis=1), want)


def check_reductions(y, x=None):
    """sum y^2 (and sum x*y) of an exact integer y: exact in any order too."""
    y = np.asarray(y, dtype=np.int64)
    check_terms((y * y)[None, :])
    assert pc.sumsq_ref(y, LD)[0] == pc.sumsq_ref(y, np.int64)[0]
    if x is not None:
        x = np.asarray(x, dtype=np.int64)
        check_terms((x * y)[None, :])
        assert pc.dot_ref(x, y, LD)[0] == pc.dot_ref(x, y, np.int64)[0]


@pytest.mark.parametrize("n", pc.GEMV_N + (pc.GEMV_TALL[1],))
def test_gemv_integer_cases(n):
    shapes = [pc.GEMV_TALL] if n == pc.GEMV_TALL[1] else pc.gemv_shapes(n)
    for m, n in shapes:
        for ep in pc.EPILOGUES:
            c = pc.gemv_case(m, n, "int", ep)
            assert np.abs(c["A"]).max() <= pc.LIM and np.array_equal(c["A"], np.rint(c["A"]))
            T = pc.gemv_terms(c, np.int64)
            check_terms(T)
            y, sumabs, nt = pc.gemv_ref(c, np.int64)
            assert np.array_equal(pc.gemv_ref(c, LD)[0], y) and nt == T.shape[1]
            assert (c["diag"] is not None) == (ep in ("diag", "both") and m == n)
            check_reductions(y, c["x"] if m == n else None)
            # the order model is one of the orders: on integer data it is exact as well
            assert np.array_equal(pc.gemv_order_model(c), y)


def test_gemvt_integer_cases():
    for m in pc.GEMVT_M:
        for n in pc.GEMVT_N:
            c = pc.gemvt_case(m, n, "int")
            check_terms(pc.gemvt_terms(c, np.int64))
            y = pc.gemvt_ref(c, np.int64)[0]
            assert np.array_equal(pc.gemvt_ref(c, LD)[0], y)
            assert np.array_equal(pc.gemvt_order_model(c), y)


@pytest.mark.parametrize("shape", pc.GRAM_SHAPES)
def test_gram_integer_cases(shape):
    m, n = shape[:2]
    A = pc.gram_case(m, n, "int")
    G, sumabs, nt = pc.gram_ref(A, np.int64)
    assert sumabs.max() < pc.TWO53 and nt == n
    assert np.array_equal(pc.gram_ref(A, LD)[0], G)
    Ai = A.astype(np.int64)
    for i in range(m):
        T = Ai[i][None, :] * Ai                                  # row i of G, term by term
        Tf = T.astype(np.float64)
        assert np.array_equal(np.cumsum(Tf, axis=1)[:, -1], G[i])
        assert np.array_equal(np.cumsum(Tf[:, ::-1], axis=1)[:, -1], G[i])


@pytest.mark.parametrize("shape", [(3000, 3000), (3000, 4000)])
def test_spmv_integer_cases(shape):
    M = pc.spmv_matrix("int", *shape)
    nnz = np.diff(M.indptr)
    # the three branches: a row beyond the tile, a run of empty rows longer than a tile holds,
    # short rows with empty ones in between
    assert nnz.max() > 2048 and np.count_nonzero(nnz > 2048) == 1
    run = np.flatnonzero(nnz[1500:2600] == 0)
    assert len(run) == 1100 and (nnz == 0).sum() > 1100 + 200
    assert M.has_sorted_indices and np.all(np.abs(M.data) <= 31)
    ops = pc.spmv_operands("int", *shape)
    x = ops["x"]
    # row sums: scipy's in-order float64 sum, the reversed rows and int64
    Mi = sps.csr_matrix((M.data.astype(np.int64), M.indices, M.indptr), shape=M.shape)
    want = Mi.dot(x.astype(np.int64))
    rev = np.concatenate([np.arange(a, b)[::-1] for a, b in zip(M.indptr[:-1], M.indptr[1:])])
    Mr = sps.csr_matrix((M.data[rev], M.indices[rev], M.indptr), shape=M.shape)
    assert np.array_equal(M.dot(x), want) and np.array_equal(Mr.dot(x), want)
    for xrow in ((x, ops["xrow"]) if shape[0] == shape[1] else (ops["xrow"],)):
        for has_diag in (False, True):
            for has_yin in (False, True):
                y, sumabs, nt = pc.spmv_ref(M, ops, has_diag, has_yin, xrow, np.int64)
                assert sumabs.max() < pc.TWO53
                assert np.array_equal(pc.spmv_ref(M, ops, has_diag, has_yin, xrow, LD)[0], y)
                yf = ops["alpha"] * M.dot(x)
                if has_diag:
                    yf = yf + ops["diag"] * xrow
                if has_yin:
                    yf = yf + ops["beta"] * ops["yin"]
                assert np.array_equal(yf, y)
                check_reductions(y, xrow)


def test_vector_integer_cases():
    for n in pc.VEC_N:
        x, y = pc.vec_ints(n, 1), pc.vec_ints(n, 2)
        check_terms((x.astype(np.int64) * y.astype(np.int64))[None, :])
        check_reductions(x)


def test_bound_and_bits_helpers():
    ok, ratio = pc.within([1.0 + 2.0 ** -52], [1.0], 1, [1.0])
    assert ok and 0 < ratio < 1                         # one ulp of 1 against (1 + 4) 2^-53
    assert not pc.within([1.0 + 2.0 ** -49], [1.0], 1, [1.0])[0]
    assert pc.same_bits([0.0, np.nan], [0.0, np.nan]) and not pc.same_bits([0.0], [-0.0])
    assert pc.same_values([0.0, np.nan], [-0.0, np.nan]) and not pc.same_values([np.nan], [1.0])
    a = pc.with_special(np.ones(5), np.inf)
    assert np.array_equal(np.flatnonzero(np.isinf(a)), [0, 2, 4])
