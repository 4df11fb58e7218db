"""Inputs, CPU references and the redzone helper of the primitive-kernel tests
(test_gpu_dense_matvec.py, test_gpu_spmv_epilogue.py, test_gpu_vec_contracts.py; the
generators themselves are checked by test_primitive_cases_host.py).  Nothing here needs a GPU
except ``Guarded``, which imports torch when it is used.

Integer-valued cases: entries are integers of magnitude <= 1023 stored as float64, scalars are
small integers, and the sizes keep the sum of |terms| of every output below 2^53 -- every
product and every partial sum in ANY order is then an integer float64 holds exactly, so a
correct kernel returns the int64 result bit for bit whatever its summation order
(``np.array_equal``, zero tolerance: a dropped, doubled or misplaced element fails).

Real-valued cases: the reference is computed in ``np.longdouble`` and the bound is the worst
case of any summation order with separately rounded or fused products,
``|got - ref| <= (n + 4) 2^-53 sum_i |a_i||x_i|`` per output with n the number of terms (the
epilogue's terms counted in both n and the sum); ``slack`` = 4, or the number of K splits for
the Gram kernel.
"""
import numpy as np

U = 2.0 ** -53
TWO53 = 2 ** 53
LIM = 1023
# what the slack around every output view is filled with: a quiet NaN whose payload no kernel
# produces, so both "written" and "consumed as an operand" show
SENTINEL = np.uint64(0x7FF8C0DEC0DEC0DE)

_LD = np.longdouble


def ints(rng, shape, lim=LIM):
    return rng.integers(-lim, lim + 1, shape).astype(np.float64)


def wide(rng, shape):
    """Normal deviates whose magnitudes span 1e-150 .. 1e150."""
    return rng.standard_normal(shape) * 10.0 ** rng.uniform(-150.0, 150.0, shape)


def bound(nterms, sumabs, slack=4):
    """(nterms + slack) 2^-53 sum|terms|, as float64 rounded up a little (the bound itself is
    formed in longdouble)."""
    return np.asarray((nterms + slack) * _LD(U) * np.asarray(sumabs, dtype=_LD) * (1 + _LD(2.0) ** -40),
                      dtype=_LD)


def within(got, ref, nterms, sumabs, slack=4):
    """(ok, worst ratio |got - ref| / bound over the outputs with a non-zero bound)."""
    err = np.abs(np.asarray(got, dtype=_LD) - np.asarray(ref, dtype=_LD))
    b = bound(nterms, sumabs, slack)
    ok = bool(np.all(err <= b))
    nz = b > 0
    ratio = float(np.max(err[nz] / b[nz])) if np.any(nz) else 0.0
    return ok, ratio


# ---------------------------------------------------------------- dense matvec
GEMV_N = (1, 63, 64, 65, 511, 512, 513, 576, 1025)
GEMV_M = (1, 3, 4, 5, 130)
GEMV_TALL = (8197, 3)              # past the 2048-workgroup cap (8192 rows)
GEMVT_M = (0, 1, 3, 4, 5, 12, 13, 15, 16, 17, 19, 20, 33)
GEMVT_N = (1, 63, 64, 65, 130)
EPILOGUES = ("none", "diag", "yin", "both")


def gemv_shapes(n):
    """The (m, n) pairs of one column count: every row count, and the square shape (diag and
    sum x*y exist only there)."""
    return [(m, n) for m in GEMV_M] + ([(n, n)] if n not in GEMV_M else [])


def gemv_case(m, n, kind, epilogue, seed=0):
    """Operands of y = alpha A x [+ diag x] [+ beta yin]; ``kind``: 'int', 'real' or 'wide'.
    diag only for square shapes (the entry refuses it otherwise)."""
    rng = np.random.default_rng([m, n, seed, EPILOGUES.index(epilogue)])
    has_diag = epilogue in ("diag", "both") and m == n
    has_yin = epilogue in ("yin", "both")
    if kind == "int":
        # x small enough that sum_r y_r^2 stays exact too (test_primitive_cases_host.py)
        A, x = ints(rng, (m, n)), ints(rng, n, 31)
        diag = ints(rng, m) if has_diag else None
        yin = ints(rng, m) if has_yin else None
        alpha, beta = (-2.0, 4.0) if (m + n) % 2 else (1.0, -1.0)
    else:
        gen = wide if kind == "wide" else (lambda r, s: r.standard_normal(s))
        A, x = gen(rng, (m, n)), rng.standard_normal(n)
        diag = rng.standard_normal(m) if has_diag else None
        yin = gen(rng, m) if has_yin else None
        alpha, beta = -1.25, 0.75
    return dict(m=m, n=n, A=A, x=x, alpha=alpha, diag=diag, beta=beta if has_yin else 0.0,
                yin=yin)


def gemv_terms(c, dtype):
    """The terms of every output as an (m, nterms) array of ``dtype``: alpha A[r][k] x[k], then
    diag[r] x[r], then beta yin[r]."""
    A, x = c["A"].astype(dtype), c["x"].astype(dtype)
    cols = [dtype(c["alpha"]) * A * x[None, :]]
    if c["diag"] is not None:
        cols.append((c["diag"].astype(dtype) * x[:c["m"]])[:, None])
    if c["yin"] is not None:
        cols.append((dtype(c["beta"]) * c["yin"].astype(dtype))[:, None])
    return np.concatenate(cols, axis=1)


def gemv_ref(c, dtype):
    """(y, sum|terms| per output, nterms)."""
    t = gemv_terms(c, dtype)
    return t.sum(axis=1), np.abs(t).sum(axis=1), t.shape[1]


def gemvt_case(m, n, kind, seed=0):
    rng = np.random.default_rng([m, n, seed, 77])
    if kind == "int":
        return dict(m=m, n=n, B=ints(rng, (m, n)), x=ints(rng, m))
    gen = wide if kind == "wide" else (lambda r, s: r.standard_normal(s))
    return dict(m=m, n=n, B=gen(rng, (m, n)), x=rng.standard_normal(m))


def gemvt_terms(c, dtype):
    return (c["B"].astype(dtype) * c["x"].astype(dtype)[:, None]).T.copy()     # (n, m)


def gemvt_ref(c, dtype):
    t = gemvt_terms(c, dtype)
    return t.sum(axis=1), np.abs(t).sum(axis=1), t.shape[1]


def sumsq_ref(y, dtype):
    """(sum y^2, sum |y^2|, nterms) of the values a kernel itself produced."""
    t = np.asarray(y).astype(dtype) ** 2
    return t.sum(), t.sum(), t.size


def dot_ref(x, y, dtype):
    t = np.asarray(x).astype(dtype) * np.asarray(y).astype(dtype)
    return t.sum(), np.abs(t).sum(), t.size


# ---- order models: every product and every sum rounded once (-ffp-contract=off)
def _tree16(v):
    """Balanced in-order pairwise sum over the last axis (16 entries)."""
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def gemv_order_model(c):
    """k_dense_gemv: lane l sums the products of columns l, l + 64, ... left to right; the wave
    sum is the in-order pairwise tree over each row of 16 lanes (IPX_WAVE_REDUCE: xor 1, xor 2,
    half-row mirror, row mirror), the four rows as (r0 + r1) + (r2 + r3); then alpha * s,
    + diag x, + beta yin, each rounded."""
    A, x, m, n = c["A"], c["x"], c["m"], c["n"]
    K = (n + 63) // 64
    P = np.zeros((m, K * 64))
    P[:, :n] = A * x[None, :]              # (a padding product is +0.0: s + 0.0 == s, s never -0.0)
    P = P.reshape(m, K, 64)
    s = np.zeros((m, 64))
    for k in range(K):
        s = s + P[:, k, :]
    rows = _tree16(s.reshape(m, 4, 16))
    y = c["alpha"] * ((rows[:, 0] + rows[:, 1]) + (rows[:, 2] + rows[:, 3]))
    if c["diag"] is not None:
        y = y + c["diag"] * x[:m]
    if c["yin"] is not None:
        y = y + c["beta"] * c["yin"]
    return y


def gemvt_order_model(c):
    """k_dense_gemvt: wave g sums the products of rows g, g + 4, ... in order; the four wave
    sums combine as ((p0 + p1) + p2) + p3."""
    B, x, m, n = c["B"], c["x"], c["m"], c["n"]
    P = B * x[:, None]
    p = np.zeros((4, n))
    for r in range(m):
        p[r % 4] = p[r % 4] + P[r]
    return ((p[0] + p[1]) + p[2]) + p[3]


# ---------------------------------------------------------------- Gram
# (m, n, lda, base offset in doubles): one chunk and empty splits; two tile rows and uneven
# chunks; n no multiple of 32 with odd lda (scalar loads); m one past a tile; odd lda; lda > n
# with an odd base (scalar loads); lda > n on the 16-byte form
GRAM_SHAPES = ((3, 8, 8, 0), (70, 100, 100, 0), (64, 33, 33, 0), (65, 64, 64, 2),
               (130, 1001, 1001, 0), (70, 96, 131, 1), (70, 96, 98, 2))
GRAM_SPLITS = (2, 3, 8)


def gram_case(m, n, kind):
    rng = np.random.default_rng([m, n, 5])
    return ints(rng, (m, n)) if kind == "int" else rng.standard_normal((m, n))


def gram_ref(A, dtype):
    """(A A', |A| |A|', n)."""
    a = A.astype(dtype)
    return a @ a.T, np.abs(a) @ np.abs(a).T, A.shape[1]


# ---------------------------------------------------------------- CSR
def spmv_matrix(kind, nrows=3000, ncols=3000, tile_nnz=2048, seed=3):
    """A CSR matrix of ``nrows`` rows with what the three branches of k_csr_spmv need: short
    rows of 0..9 entries, empty rows sprinkled in, a run of 1100 empty rows (more than the 1024
    rows a tile may hold: a tile filled by its row count), and one row of tile_nnz + 150 entries
    (a tile of its own on the long-row branch).  Column indices sorted, no repeats."""
    import scipy.sparse as sps
    rng = np.random.default_rng([seed, nrows, ncols])
    long_row, run0 = 700, 1500
    indptr, indices = [0], []
    for r in range(nrows):
        if r == long_row:
            k = min(tile_nnz + 150, ncols)
        elif run0 <= r < run0 + 1100 or r % 7 == 3:
            k = 0
        else:
            k = int(rng.integers(0, 10))
        indices.append(np.sort(rng.choice(ncols, size=k, replace=False)))
        indptr.append(indptr[-1] + k)
    indices = np.concatenate(indices).astype(np.int32)
    # the long row sums 2198 products: entries <= 31 there keep sum y^2 exact as well
    data = ints(rng, len(indices), 31) if kind == "int" else rng.standard_normal(len(indices))
    return sps.csr_matrix((data, indices, np.asarray(indptr, dtype=np.int32)),
                          shape=(nrows, ncols))


def spmv_operands(kind, nrows, ncols, seed=4):
    rng = np.random.default_rng([seed, nrows, ncols])
    gen = (lambda s: ints(rng, s, 31)) if kind == "int" else rng.standard_normal
    return dict(x=gen(ncols), xrow=gen(nrows), diag=gen(nrows), yin=gen(nrows),
                alpha=-2.0 if kind == "int" else -1.25, beta=4.0 if kind == "int" else 0.75)


def spmv_ref(M, ops, has_diag, has_yin, xrow, dtype):
    """(y, sum|terms| per row, terms per row) with the row sums taken in ``dtype``."""
    import scipy.sparse as sps
    Md = sps.csr_matrix((M.data.astype(dtype), M.indices, M.indptr), shape=M.shape)
    Ma = sps.csr_matrix((np.abs(M.data).astype(dtype), M.indices, M.indptr), shape=M.shape)
    x = ops["x"].astype(dtype)
    alpha, beta = dtype(ops["alpha"]), dtype(ops["beta"])
    y = alpha * _csr_dot(Md, x)
    sa = abs(alpha) * _csr_dot(Ma, np.abs(x))
    nt = np.diff(M.indptr).astype(np.int64)
    if has_diag:
        t = ops["diag"].astype(dtype) * xrow.astype(dtype)
        y, sa, nt = y + t, sa + np.abs(t), nt + 1
    if has_yin:
        t = beta * ops["yin"].astype(dtype)
        y, sa, nt = y + t, sa + np.abs(t), nt + 1
    return y, sa, nt


def _csr_dot(M, x):
    """M x with the row sums in M's dtype (scipy has no longdouble kernels: per-row numpy)."""
    if M.dtype != np.longdouble:
        return M.dot(x)
    prod = M.data * x[M.indices]
    out = np.zeros(M.shape[0], dtype=np.longdouble)
    nz = np.flatnonzero(np.diff(M.indptr))
    out[nz] = np.add.reduceat(prod, M.indptr[nz]) if len(nz) else 0
    return out


# ---------------------------------------------------------------- vectors
VEC_N = (1, 2, 255, 256, 257, 1023, 1025, (1 << 20) + 3)
SPECIALS = (np.nan, np.inf, -np.inf, -0.0, 5e-324, 1.797e308)


def vec_ints(n, seed):
    return ints(np.random.default_rng([n, seed]), n)


def special_positions(n):
    return sorted({0, n // 2, n - 1})


def with_special(a, value):
    """A copy of ``a`` with ``value`` at the first, an interior and the last position."""
    a = np.array(a, dtype=np.float64)
    a[special_positions(len(a))] = value
    return a


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_values(a, b):
    """Equal as numbers (-0.0 == +0.0), NaN where and only where the other has one."""
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# ---------------------------------------------------------------- redzones
class Guarded:
    """A host array as a view into a larger device buffer: ``offset`` doubles of slack in front
    (even / odd: the 16-byte / 8-byte forms of the kernels that switch on pointer parity),
    ``tail`` behind and, for a matrix with leading dimension ``lda`` > its column count,
    between the rows.  The slack holds ``fill``: SENTINEL around an output, NaN or 0.0 around an
    input (a kernel that consumes a neighbour's value gives different bits for the two).
    ``read()`` returns the view's contents after checking that every slack byte is unchanged.
    Every pointer stays inside the buffer by construction; accesses that land in foreign
    memory are not detected (and nothing tries to provoke one)."""

    def __init__(self, a, offset=1, tail=9, fill=None, lda=None):
        import torch
        a = np.asarray(a, dtype=np.float64)
        self.shape, self.offset = a.shape, offset
        if a.ndim == 2:
            m, n = a.shape
            self.lda = n if lda is None else lda
            assert self.lda >= n
            span = (m - 1) * self.lda + n if m else 0
            idx = (np.arange(m)[:, None] * self.lda + np.arange(n)[None, :]).reshape(-1)
        else:
            assert lda is None
            span = a.size
            idx = np.arange(span)
        buf = np.empty(offset + span + tail, dtype=np.float64)
        if fill is None:
            buf.view(np.uint64)[:] = SENTINEL
        else:
            buf[:] = fill
        self.idx = offset + idx
        buf[self.idx] = a.reshape(-1)
        self.mask = np.zeros(buf.size, dtype=bool)
        self.mask[self.idx] = True
        self.before = buf.copy()
        self.t = torch.from_numpy(buf).cuda()
        self.ptr = self.t.data_ptr() + 8 * offset

    @classmethod
    def output(cls, shape, offset=1, tail=9, lda=None):
        """An output view pre-filled, like its slack, with the sentinel."""
        a = np.empty(shape, dtype=np.float64)
        a.view(np.uint64)[...] = SENTINEL
        return cls(a, offset, tail, None, lda)

    def tensor(self):
        """The view of a vector as a device tensor (for the package's DVec)."""
        assert len(self.shape) == 1
        return self.t[self.offset:self.offset + self.shape[0]]

    def read(self):
        after = self.t.cpu().numpy()
        out = ~self.mask
        assert np.array_equal(after.view(np.uint64)[out], self.before.view(np.uint64)[out]), \
            "a kernel wrote outside its view"
        return after[self.idx].reshape(self.shape)
