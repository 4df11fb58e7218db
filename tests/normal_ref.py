"""Exact references for the device assembly of the normal matrix ``A A'`` (and its weighted,
banded, padded and block forms), for tests/test_gpu_normal_assembly.py.

Two input classes make the reference exact, so that a kernel is judged entry by entry:

* ``int_values``: integers with |a| <= 2**10.  With at most a few thousand columns every
  product and every partial sum is an integer below 2**53: any summation order gives the same
  bits, and the device result must equal the int64 reference exactly.
* ``bits26_values``: random values rounded to 26 significant bits (of varying magnitude).
  Every product of two of them is exact in fp64, so ``math.fsum`` of the products is the
  correctly rounded ``(A A')_ij``; a computed entry must lie within ``gamma_k * sum_t |a_it a_jt|``
  of it, k the number of products (``within_bound``).  A small entry has a small bound.

Nothing here needs a GPU.
"""
import math

import numpy as np
import scipy.sparse as sps

U = 2.0 ** -53                        # unit roundoff of fp64


def gamma(k):
    """gamma_k = k u / (1 - k u): the componentwise error bound of a k-term sum of exact
    products, in any order (Higham, Accuracy and Stability, 2nd ed., section 3.1)."""
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


def int_values(rng, size, lim=2 ** 10):
    """Non-zero integers in [-lim, lim] (as float64)."""
    v = rng.integers(1, lim + 1, size) * rng.choice((-1, 1), size)
    return v.astype(np.float64)


def round_bits(x, bits):
    """x rounded to ``bits`` significant bits."""
    mant, ex = np.frexp(np.asarray(x, dtype=np.float64))
    return np.ldexp(np.round(np.ldexp(mant, bits)), ex - bits)


def bits26_values(rng, size, spread=8, bits=26):
    """Normal random values times 2**e, e uniform in [-spread, spread], rounded to ``bits``
    significant bits: products of two are exact in fp64, the magnitudes vary."""
    x = rng.standard_normal(size) * np.ldexp(1.0, rng.integers(-spread, spread + 1, size))
    x = round_bits(x, bits)
    x[x == 0] = 1.0
    return x


def random_csr(rng, m, n, lengths, values):
    """m x n canonical CSR with ``lengths[i]`` distinct random columns in row i, values drawn by
    ``values(rng, nnz)``."""
    lengths = np.minimum(np.asarray(lengths, dtype=np.int64), n)
    rows = [np.sort(rng.choice(n, int(L), replace=False)) for L in lengths]
    indptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
    indices = (np.concatenate(rows) if rows else np.zeros(0)).astype(np.int32)
    return sps.csr_matrix((values(rng, int(indptr[-1])), indices, indptr), shape=(m, n))


def split_duplicates(A):
    """The same matrix with every stored value v replaced by two adjacent entries v/2, v/2 in
    the same (row, column): scipy reads it as A (v/2 + v/2 == v exactly), but it is not in
    canonical format."""
    A = sps.csr_matrix(A)
    A.sort_indices()
    indptr = (2 * A.indptr).astype(np.int32)
    indices = np.repeat(A.indices, 2).astype(np.int32)
    data = np.repeat(A.data * 0.5, 2)
    D = sps.csr_matrix((data, indices, indptr), shape=A.shape)
    assert not D.has_canonical_format or A.nnz == 0
    return D


# ---------------------------------------------------------------- the reference entries
def _rows(A):
    A = sps.csr_matrix(A)
    return [(A.indices[A.indptr[i]:A.indptr[i + 1]], A.data[A.indptr[i]:A.indptr[i + 1]])
            for i in range(A.shape[0])]


def pair_products(ci, vi, cj, vj, wcol=None):
    """The exact products a_it a_jt [w_t] over the columns common to two canonical rows."""
    common, pi, pj = np.intersect1d(ci, cj, assume_unique=True, return_indices=True)
    p = vi[pi] * vj[pj]
    if wcol is not None:
        p = p * wcol[common]
    return p


def entry(rows, i, j, wcol=None):
    """(correctly rounded (A W A')_ij, sum |products|, number of products).  Exact as long as
    every product is (see the input classes; with ``wcol`` the caller keeps a * a * w exact)."""
    ci, vi = rows[i]
    cj, vj = rows[j]
    p = pair_products(ci, vi, cj, vj, wcol)
    return math.fsum(p), math.fsum(np.abs(p)), len(p)


def gram_int(A_dense):
    """A A' of an integer-valued dense matrix, exactly (int64)."""
    Ai = np.asarray(A_dense).astype(np.int64)
    assert np.array_equal(Ai, A_dense)
    return Ai @ Ai.T


def aat_int(A, wcol=None):
    """A W A' of an integer-valued CSR matrix (integer weights), exactly, as a dense int64."""
    A = sps.csr_matrix(A)
    Ai = sps.csr_matrix((A.data.astype(np.int64), A.indices, A.indptr), shape=A.shape)
    assert np.array_equal(Ai.data, A.data)
    if wcol is not None:
        w = np.asarray(wcol).astype(np.int64)
        assert np.array_equal(w, wcol)
        B = Ai.multiply(w[None, :]).tocsr()
    else:
        B = Ai
    return np.asarray(B.dot(Ai.T).toarray(), dtype=np.int64)


def band_of(S, perm, k):
    """band[d, i] = S[p_i, p_{i-d}] (0 where i - d < 0): the band storage of the device."""
    m = S.shape[0]
    p = np.arange(m) if perm is None else np.asarray(perm)
    out = np.zeros((k + 1, m), dtype=S.dtype)
    for d in range(k + 1):
        out[d, d:] = S[p[d:], p[:m - d]]
    return out


def band_fsum(A, perm, k, wcol=None):
    """(value, sum |products|, count) arrays of shape (k+1, m) for the band storage by fsum."""
    rows = _rows(A)
    m = A.shape[0]
    p = np.arange(m) if perm is None else np.asarray(perm)
    val, mag, cnt = (np.zeros((k + 1, m)), np.zeros((k + 1, m)), np.zeros((k + 1, m), np.int64))
    for d in range(k + 1):
        for i in range(d, m):
            val[d, i], mag[d, i], cnt[d, i] = entry(rows, p[i], p[i - d], wcol)
    return val, mag, cnt


def gram_fsum_dense(A_dense):
    """(value, sum |products|) of A A' for a dense matrix whose products are exact: lower
    triangle by fsum, mirrored."""
    m = A_dense.shape[0]
    val, mag = np.zeros((m, m)), np.zeros((m, m))
    for i in range(m):
        P = A_dense[i][None, :] * A_dense[:i + 1]          # exact products, rows j <= i
        for j in range(i + 1):
            val[i, j] = val[j, i] = math.fsum(P[j])
            mag[i, j] = mag[j, i] = math.fsum(np.abs(P[j]))
    return val, mag


def gram_fsum_csr(A):
    """(value, sum |products|, count) of A A' for a CSR matrix with exact products."""
    rows = _rows(A)
    m = A.shape[0]
    val, mag, cnt = np.zeros((m, m)), np.zeros((m, m)), np.zeros((m, m), np.int64)
    for i in range(m):
        for j in range(i + 1):
            v, s, c = entry(rows, i, j)
            val[i, j] = val[j, i] = v
            mag[i, j] = mag[j, i] = s
            cnt[i, j] = cnt[j, i] = c
    return val, mag, cnt


def within_bound(got, val, mag, k):
    """Boolean mask of the entries with |got - val| <= gamma_k * mag (k per entry or scalar;
    an entry of one product, or none, must be exact)."""
    return np.abs(np.asarray(got) - val) <= gamma(k) * mag


def worst(got, val, mag, k):
    """The entry furthest outside the bound, for assertion messages."""
    excess = np.abs(np.asarray(got) - val) - gamma(k) * mag
    idx = np.unravel_index(np.argmax(excess), np.shape(excess))
    return idx, np.asarray(got)[idx], val[idx], float(np.max(excess))


# ------------------------------------------------- solves with S = A A': exact residuals
# A = diag(2^e) A_int with A_int integer: every product a_it a_jt is an integer times
# 2^(e_i + e_j), so S = A A' is exactly representable, the device assembles it exactly (any
# summation order), and the residual r = w - S v of a computed solve is evaluated exactly.
def pow2_rows(A_int, e):
    """diag(2^e) A_int, exactly (CSR)."""
    A = sps.csr_matrix(A_int, copy=True)
    A.data = np.ldexp(A.data, np.repeat(np.asarray(e, dtype=np.int64), np.diff(A.indptr)))
    return A


def gram_pow2(A_int, e=None):
    """S = A A' of A = diag(2^e) A_int as a CSR float64 matrix, exactly: the int64 product of
    the integer rows, each entry times 2^(e_i + e_j) (both steps checked)."""
    A = sps.csr_matrix(A_int)
    Ai = sps.csr_matrix((A.data.astype(np.int64), A.indices, A.indptr), shape=A.shape)
    assert np.array_equal(Ai.data, A.data), "A_int is not integer-valued"
    S = (Ai @ Ai.T).tocoo()
    assert S.nnz == 0 or np.abs(S.data).max() < 2 ** 53
    e = np.zeros(A.shape[0], np.int64) if e is None else np.asarray(e, dtype=np.int64)
    ex = e[S.row] + e[S.col]
    val = np.ldexp(S.data.astype(np.float64), ex)
    assert np.array_equal(np.ldexp(val, -ex), S.data.astype(np.float64)), \
        "S is not exactly representable"
    out = sps.csr_matrix((val, (S.row, S.col)), shape=S.shape)
    out.sort_indices()
    return out


def split26(v):
    """Veltkamp's split v = hi + lo (exactly), both halves of at most 26 significant bits."""
    v = np.asarray(v, dtype=np.float64)
    c = v * 134217729.0                                      # 2^27 + 1
    hi = c - (c - v)
    return hi, v - hi


def assert_26_bits(x):
    """Every entry is an integer below 2^26 times a power of two (or 0)."""
    mant, _ = np.frexp(np.asarray(x, dtype=np.float64))
    scaled = np.ldexp(mant, 26)
    assert np.array_equal(scaled, np.round(scaled)), "an entry has more than 26 significant bits"


def residual_exact(S, v, w):
    """r = w - S v with every entry correctly rounded.  S_ij has at most 26 significant bits
    (asserted) and v_j is split into two halves of 26 bits, so every S_ij v_half is exact and
    ``math.fsum`` of w_i and the products of row i is the correctly rounded r_i."""
    S = sps.csr_matrix(S)
    assert_26_bits(S.data)
    v = np.asarray(v, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    hi, lo = split26(v)
    assert np.array_equal(hi + lo, v)
    ph = (-S.data * hi[S.indices]).tolist()
    pl = (-S.data * lo[S.indices]).tolist()
    ip = S.indptr.tolist()
    wl = w.tolist()
    return np.array([math.fsum([wl[i]] + ph[ip[i]:ip[i + 1]] + pl[ip[i]:ip[i + 1]])
                     for i in range(S.shape[0])])


def pow2_scale(S):
    """f with Delta = diag(2^f), f_i = floor(log2 sqrt(S_ii) + 1/2): powers of two, so the
    scaled system (Delta^-1 S Delta^-1)(Delta v) = Delta^-1 w is formed without rounding, and
    rows scaled by 2^e shift f by e exactly."""
    d = np.asarray(sps.csr_matrix(S).diagonal(), dtype=np.float64)
    assert np.all(d > 0)
    return np.floor(0.5 * np.log2(d) + 0.5).astype(np.int64)


def scaled_matrix(S):
    """Delta^-1 S Delta^-1 (CSR), exact."""
    S = sps.csr_matrix(S)
    f = pow2_scale(S)
    rows = np.repeat(np.arange(S.shape[0]), np.diff(S.indptr))
    return sps.csr_matrix((np.ldexp(S.data, -(f[rows] + f[S.indices])), S.indices, S.indptr),
                          shape=S.shape)


def backward_error(S, v, w, r=None):
    """Normwise backward error of v for the diagonally scaled system (Delta: pow2_scale),
        eta = ||D^-1 r||_inf / (||D^-1 S D^-1||_inf ||D v||_inf + ||D^-1 w||_inf),
    r the exact residual (residual_exact, or given).  Rows of A scaled by powers of two change
    it only through rounding."""
    S = sps.csr_matrix(S)
    if r is None:
        r = residual_exact(S, v, w)
    f = pow2_scale(S)
    normS = float(np.max(np.asarray(abs(scaled_matrix(S)).sum(axis=1)).ravel()))
    num = float(np.max(np.abs(np.ldexp(r, -f))))
    den = normS * float(np.max(np.abs(np.ldexp(v, f)))) + \
        float(np.max(np.abs(np.ldexp(w, -f))))
    return num / den if den > 0 else 0.0


def scaled_cond(S):
    """kappa_2(Delta^-1 S Delta^-1), host float64 (dense: for the sizes the dense solver takes)."""
    ev = np.linalg.eigvalsh(scaled_matrix(S).toarray())
    return float(ev[-1] / ev[0])
