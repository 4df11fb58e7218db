"""The device assembly of the normal matrix A A' against an exact reference (tests/normal_ref.py),
entry by entry, through the C ABI:

  ipx_aat_band_w            band storage, staged (k_aat_band_rows) and global joins, a row order
  ipx_gram_f64_mfma_split   dense A A' on the matrix cores, K split in explicit pieces
  ipx_aat_dense             dense A A' of a CSR matrix (padded layout)
  ipx_blockjacobi_build     32 x 32 diagonal blocks of A A' in a row order, inverted
  ipx_blockjacobi_apply     z = M^-1 r by those blocks, and its r'z partials

Integer inputs must come out bit-exact; inputs rounded to 26 bits within gamma_k * sum |a a'|
per entry.  Then: a Jacobian that stores its entries twice (v/2 + v/2) gives bit-identical
solves to the canonical one, and a device pattern with a repeated entry is refused."""
import math

import numpy as np
import pytest
import scipy.sparse as sps

import normal_ref as nr

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def env():
    import torch
    from ipsolver import _hip, device as dv
    return _hip, dv, torch


def _t(torch, a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def _csr_dev(torch, A):
    return (_t(torch, A.indptr, np.int32), _t(torch, A.indices, np.int32),
            _t(torch, A.data if A.nnz else np.zeros(1), np.float64))


# ------------------------------------------------------------------------ ipx_aat_band_w
def _band_matrix(rng, m, k, values, long_rows, narrow=False):
    """Rows of 0..5 entries (empty and single-entry rows among them) in a window that moves
    two columns per row, so neighbouring rows share columns; with ``long_rows`` the rows of
    the second group of 256 carry 30..40 entries -- their workgroup's piece of the CSR arrays
    exceeds AAT_CAP and takes the global join in the same launch as the staged ones.
    ``narrow``: every row in the same 48 columns (rows in any order overlap)."""
    lengths = rng.integers(0, 6, m)
    lengths[:min(m, 3)] = (0, 1, 2)[:min(m, 3)]
    if long_rows:
        lengths[256:512] = rng.integers(30, 41, len(lengths[256:512]))
    width = 48 if narrow else 60
    n = width if narrow else 2 * m + width
    rows = []
    for i in range(m):
        lo = 0 if narrow else 2 * i
        rows.append(np.sort(rng.choice(np.arange(lo, lo + width), int(lengths[i]), replace=False)))
    indptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
    indices = np.concatenate(rows).astype(np.int32) if indptr[-1] else np.zeros(0, np.int32)
    return sps.csr_matrix((values(rng, int(indptr[-1])), indices, indptr), shape=(m, n))


def _run_band(env, A, k, perm, wcol):
    _hip, dv, torch = env
    m = A.shape[0]
    band = torch.full(((k + 1) * m,), NAN, dtype=torch.float64, device="cuda")
    ip, ix, v = _csr_dev(torch, A)
    pd = _t(torch, perm, np.int32) if perm is not None else None
    wd = _t(torch, wcol, np.float64) if wcol is not None else None
    _hip.call("ipx_aat_band_w", m, k, dv._p(ip), dv._p(ix), dv._p(v), dv._p(pd), dv._p(wd),
              dv._p(band), dv.stream_ptr())
    got = band.cpu().numpy().reshape(k + 1, m)
    assert not np.isnan(got).any(), "a band slot was not written"
    for d in range(k + 1):                 # the slots before the first row of a diagonal
        assert np.array_equal(got[d, :d], np.zeros(min(d, m))) and \
            not np.signbit(got[d, :d]).any()
    return got


# m: one row, one workgroup short / exact / one over, two workgroups +- 1 row
BAND_CASES = [(1, 0), (1, 3), (255, 1), (256, 2), (257, 8), (511, 4), (513, 5), (513, 8),
              (300, 0), (257, 6), (511, 7), (256, 3)]


@pytest.mark.parametrize("m,k", BAND_CASES)
@pytest.mark.parametrize("order", ["identity", "perm"])
@pytest.mark.parametrize("weighted", [False, True])
def test_aat_band_integer_exact(env, m, k, order, weighted):
    """Integer entries: the band equals the int64 reference bit for bit -- identity order
    (k_aat_band_rows: staged pieces, and with m > 256 a group of long rows whose workgroup
    joins out of global memory in the same launch) and a random order (k_aat_band)."""
    rng = np.random.default_rng(1000 * m + 10 * k + 2 * weighted + (order == "perm"))
    A = _band_matrix(rng, m, k, nr.int_values, long_rows=m > 256, narrow=order == "perm")
    perm = rng.permutation(m).astype(np.int32) if order == "perm" else None
    wcol = nr.int_values(rng, A.shape[1], 2 ** 8) if weighted else None
    got = _run_band(env, A, k, perm, wcol)
    want = nr.band_of(nr.aat_int(A, wcol), perm, k)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("m,k", [(1, 2), (255, 3), (257, 8), (513, 5), (513, 8)])
@pytest.mark.parametrize("order", ["identity", "perm"])
@pytest.mark.parametrize("weighted", [False, True])
def test_aat_band_bits26_within_bound(env, m, k, order, weighted):
    """Values of varying magnitude rounded to 26 bits (20 bits against 13-bit column weights,
    so a * a * w stays exact): every band entry within gamma_k * sum |products| of the
    correctly rounded value, k the number of products of that entry."""
    rng = np.random.default_rng(7000 + 1000 * m + 10 * k + 2 * weighted + (order == "perm"))
    bits = 20 if weighted else 26
    A = _band_matrix(rng, m, k, lambda r, s: nr.bits26_values(r, s, bits=bits),
                     long_rows=m > 256, narrow=order == "perm")
    perm = rng.permutation(m).astype(np.int32) if order == "perm" else None
    wcol = nr.round_bits(rng.uniform(0.25, 4.0, A.shape[1]), 13) if weighted else None
    got = _run_band(env, A, k, perm, wcol)
    val, mag, cnt = nr.band_fsum(A, perm, k, wcol)
    ok = nr.within_bound(got, val, mag, cnt)
    assert ok.all(), nr.worst(got, val, mag, cnt)


# ------------------------------------------------------------- ipx_gram_f64_mfma_split
GRAM_M = [1, 63, 64, 65, 130, 300]
GRAM_N = [0, 1, 31, 32, 33, 64, 1000, 4097]
SPLITS = [1, 2, 3, 5, 8]


def _run_gram(env, A_h, lda, splits, offset):
    """G of A_h (m x n) stored with leading dimension lda (columns past n NaN), the base
    pointer ``offset`` doubles into its buffer; G and ws prefilled with NaN."""
    _hip, dv, torch = env
    lib = _hip.load()
    m, n = A_h.shape
    buf = np.full(offset + max(m * lda, 1), NAN)
    buf[offset:offset + m * lda].reshape(m, lda)[:, :n] = A_h
    Ad = _t(torch, buf, np.float64)
    M = int(lib.ipx_dense_padded(m))
    G = torch.full((M, M), NAN, dtype=torch.float64, device="cuda")
    ws = None
    if splits > 1:
        ws = torch.full((int(lib.ipx_gram_ws_doubles(m, splits)),), NAN, dtype=torch.float64,
                        device="cuda")
    import ctypes
    ptr = ctypes.c_void_p(Ad.data_ptr() + 8 * offset)
    _hip.call("ipx_gram_f64_mfma_split", m, n, ptr, lda, dv._p(G), dv._p(ws), splits,
              dv.stream_ptr())
    Gh = G.cpu().numpy()
    assert np.array_equal(Gh, Gh.T), "not mirrored exactly"        # (NaN fails this too)
    tail = np.eye(M)
    tail[:m, :m] = Gh[:m, :m]
    assert np.array_equal(Gh, tail), "padding is not the identity"
    return Gh[:m, :m]


def _gram_layouts(n):
    """(lda, offset): packed; lda + 1 (odd -> scalar loads when n is even, and vice versa);
    lda + 5; packed but the base one double off 16 bytes (the 16-byte path refused)."""
    return [(n, 0), (n + 1, 0), (n + 5, 0), (n, 1)]


@pytest.mark.parametrize("m", GRAM_M)
@pytest.mark.parametrize("n", GRAM_N)
def test_gram_split_integer_exact(env, m, n):
    """Integer entries: every K split count (some splits empty when ceil(n/32) < splits),
    every leading dimension / alignment -- the lower triangle equals the int64 reference
    exactly, the matrix is mirrored exactly, the padding is the identity."""
    rng = np.random.default_rng(31 * m + n)
    A_h = nr.int_values(rng, (m, n)).reshape(m, n)
    want = nr.gram_int(A_h).astype(np.float64)
    for splits in SPLITS:
        for lda, off in _gram_layouts(n):
            got = _run_gram(env, A_h, lda, splits, off)
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (splits, lda, off, bad[:5])


@pytest.mark.parametrize("m", [1, 63, 65, 130])
@pytest.mark.parametrize("n", [0, 1, 33, 64, 1000])
def test_gram_split_bits26_within_bound(env, m, n):
    """26-bit values: every entry within gamma_{n + splits} * sum_t |a_it a_jt| of the correctly
    rounded (A A')_ij (any summation order of n products and the fixed-order sum of the
    split partials), every split count and layout."""
    rng = np.random.default_rng(17 * m + n + 5)
    A_h = nr.bits26_values(rng, m * n).reshape(m, n)
    val, mag = nr.gram_fsum_dense(A_h)
    for splits in SPLITS:
        for lda, off in _gram_layouts(n):
            got = _run_gram(env, A_h, lda, splits, off)
            ok = nr.within_bound(got, val, mag, n + splits)
            assert ok.all(), (splits, lda, off, nr.worst(got, val, mag, n + splits))


def test_gram_splits_contract(env):
    """ipx_gram_splits: 1..8, and 1 when the matrix is too short to split (fewer than 16 K
    chunks); ipx_gram_ws_doubles: splits x lower-triangle tiles x 64 x 64 (0 unsplit)."""
    _hip, dv, torch = env
    lib = _hip.load()
    for m in (1, 63, 64, 65, 300, 2000, 5000):
        for n in (0, 1, 31, 32, 480, 511, 512, 513, 4097, 100000):
            s = int(lib.ipx_gram_splits(m, n))
            assert 1 <= s <= 8, (m, n, s)
            if -(-n // 32) < 16:
                assert s == 1, (m, n, s)
        M = int(lib.ipx_dense_padded(m))
        assert M % 64 == 0 and m <= M < m + 64
        nt = M // 64
        for splits in range(0, 9):
            want = 0 if splits <= 1 else splits * (nt * (nt + 1) // 2) * 64 * 64
            assert int(lib.ipx_gram_ws_doubles(m, splits)) == want, (m, splits)


# ------------------------------------------------------------------------- ipx_aat_dense
def _dense_csr_matrix(rng, m, values, long_len=300):
    """Rows of 0, 1, a few and (every 16th row) ``long_len`` entries over 4 m + 400 columns."""
    n = 4 * m + 400
    lengths = rng.integers(2, 12, m)
    lengths[0::7] = 0
    lengths[3::7] = 1
    lengths[5::16] = long_len
    return nr.random_csr(rng, m, n, lengths, values)


def _run_aat_dense(env, A):
    _hip, dv, torch = env
    lib = _hip.load()
    m = A.shape[0]
    M = int(lib.ipx_dense_padded(m))
    G = torch.full((M, M), NAN, dtype=torch.float64, device="cuda")
    ip, ix, v = _csr_dev(torch, A)
    _hip.call("ipx_aat_dense", m, dv._p(ip), dv._p(ix), dv._p(v), dv._p(G), dv.stream_ptr())
    Gh = G.cpu().numpy()
    assert np.array_equal(Gh, Gh.T), "not mirrored exactly"
    tail = np.eye(M)
    tail[:m, :m] = Gh[:m, :m]
    assert np.array_equal(Gh, tail), "padding is not the identity"
    return Gh[:m, :m]


@pytest.mark.parametrize("m", [1, 63, 64, 65, 1999])
def test_aat_dense_integer_exact(env, m):
    rng = np.random.default_rng(m + 77)
    A = _dense_csr_matrix(rng, m, nr.int_values, long_len=300 if m < 1000 else 120)
    got = _run_aat_dense(env, A)
    want = nr.aat_int(A).astype(np.float64)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, bad[:5]


@pytest.mark.parametrize("m", [1, 63, 64, 65])
def test_aat_dense_bits26_within_bound(env, m):
    rng = np.random.default_rng(m + 78)
    A = _dense_csr_matrix(rng, m, nr.bits26_values)
    got = _run_aat_dense(env, A)
    val, mag, cnt = nr.gram_fsum_csr(A)
    ok = nr.within_bound(got, val, mag, cnt)
    assert ok.all(), nr.worst(got, val, mag, cnt)


# ------------------------------------------------------------ block Jacobi: build, apply
BJ = 32
C_INV = 4.0          # ||X S - I||_max <= C_INV * 32 u cond(S) for the computed inverse X
                     # (Cholesky, triangular inverse, X = L^-T L^-1; 0.03 seen on the host)


def _bj_matrix(rng, m, values):
    return nr.random_csr(rng, m, 6 * m + 40, rng.integers(3, 20, m), values)


def _bj_order(rng, m):
    nblk = -(-m // BJ)
    order = np.full(nblk * BJ, -1, dtype=np.int32)
    order[:m] = rng.permutation(m)
    return order, nblk


def _run_bj_build(env, A, order, nblk):
    _hip, dv, torch = env
    ip, ix, v = _csr_dev(torch, A)
    od = _t(torch, order, np.int32)
    binv = torch.full((nblk * BJ * BJ,), NAN, dtype=torch.float64, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    _hip.call("ipx_blockjacobi_build", nblk, dv._p(ip), dv._p(ix), dv._p(v), dv._p(od),
              dv._p(binv), dv._p(flag), dv.stream_ptr())
    return binv.cpu().numpy().reshape(nblk, BJ, BJ), int(flag.item())


def _block_refs(A, order, nblk, integer):
    """The exact 32 x 32 blocks S_b (rows order[b*32 + s]; identity rows / columns where
    order < 0), as correctly rounded doubles."""
    if integer:
        S = nr.aat_int(A).astype(np.float64)
    else:
        S, _, _ = nr.gram_fsum_csr(A)
    out = np.zeros((nblk, BJ, BJ))
    for b in range(nblk):
        o = order[b * BJ:(b + 1) * BJ]
        live = o >= 0
        Sb = np.eye(BJ)
        Sb[np.ix_(live, live)] = S[np.ix_(o[live], o[live])]
        out[b] = Sb
    return out


@pytest.mark.parametrize("m", [32, 200, 257])
@pytest.mark.parametrize("integer", [True, False])
def test_blockjacobi_build_inverts_the_blocks(env, m, integer):
    """Every block of binv is exactly symmetric, its padding rows / columns (a ragged last
    block) are the identity, and binv_b S_b = I to C_INV * 32 u cond(S_b); flag stays 0."""
    rng = np.random.default_rng(m + 11 * integer)
    A = _bj_matrix(rng, m, nr.int_values if integer else nr.bits26_values)
    order, nblk = _bj_order(rng, m)
    binv, flag = _run_bj_build(env, A, order, nblk)
    assert flag == 0
    Sb = _block_refs(A, order, nblk, integer)
    for b in range(nblk):
        X = binv[b]
        assert np.array_equal(X, X.T), b
        live = order[b * BJ:(b + 1) * BJ] >= 0
        pad = ~live
        assert np.array_equal(X[pad][:, pad], np.eye(int(pad.sum()))), b
        assert not X[pad][:, live].any() and not X[live][:, pad].any(), b
        err = np.max(np.abs(X @ Sb[b] - np.eye(BJ)))
        bound = C_INV * BJ * nr.U * np.linalg.cond(Sb[b])
        assert err <= bound, (b, err, bound)


@pytest.mark.parametrize("exact_zero", [True, False])
def test_blockjacobi_build_flags_dependent_rows(env, exact_zero):
    """Two linearly dependent rows in one block set the flag: placed first in the block with a
    perfect-square norm the second pivot is exactly 0 (bit 1); anywhere else rounding leaves
    a tiny pivot of either sign (bit 1 or bit 2, 'lost 43 bits').  The other blocks alone
    leave it 0."""
    rng = np.random.default_rng(5 + exact_zero)
    m = 96
    A = _bj_matrix(rng, m, nr.int_values if exact_zero else nr.bits26_values).tolil()
    order, nblk = _bj_order(rng, m)
    if exact_zero:
        i, j = order[BJ], order[BJ + 1]           # block 1, slots 0 and 1
        A[i] = 0
        A[i, 10] = 3.0
        A[i, 11] = 4.0
        A[j] = 2 * A[i]
    else:
        i, j = order[BJ + 9], order[BJ + 22]
        A[i] = -3 * A[j]
    A = A.tocsr()
    A.sort_indices()
    _, flag = _run_bj_build(env, A, order, nblk)
    assert flag != 0 and (flag & 1 if exact_zero else True), flag
    keep = np.concatenate((order[:BJ], order[2 * BJ:]))
    sub = np.full(2 * BJ, -1, dtype=np.int32)
    sub[:len(keep)] = keep
    _, flag = _run_bj_build(env, A, sub, 2)
    assert flag == 0


@pytest.mark.parametrize("m", [32, 200, 257])
def test_blockjacobi_apply(env, m):
    """z[order[b*32 + s]] = sum_k binv_b[s, k] r[order[b*32 + k]] within gamma_32 of the fsum
    over the device's own binv; entries of z that no block covers stay untouched; the r'z
    partials (one per workgroup, folded by the CG) sum to r'z within gamma_{m+1}."""
    _hip, dv, torch = env
    rng = np.random.default_rng(m + 3)
    A = _bj_matrix(rng, m, nr.bits26_values)
    order, nblk = _bj_order(rng, m)
    binv, flag = _run_bj_build(env, A, order, nblk)
    assert flag == 0
    r = rng.standard_normal(m + 8)
    sentinel = 1234.5
    z = torch.full((m + 8,), sentinel, dtype=torch.float64, device="cuda")
    nwg = -(-nblk // 8)
    ws = torch.full((nwg + 1,), NAN, dtype=torch.float64, device="cuda")
    state = torch.zeros(16, dtype=torch.float64, device="cuda")
    # (every buffer held by a name until the results are read: a temporary's memory goes back
    # to the allocator at once and the next upload may take it)
    od, bd, rd = (_t(torch, order, np.int32), _t(torch, binv.reshape(-1), np.float64),
                  _t(torch, r, np.float64))
    _hip.call("ipx_blockjacobi_apply", m, nblk, dv._p(od), dv._p(bd), dv._p(rd), dv._p(z),
              dv._p(ws), dv._p(state), dv.stream_ptr())
    zh, wsh = z.cpu().numpy(), ws.cpu().numpy()
    assert np.all(zh[m:] == sentinel)                    # rows m.. belong to no block
    want, mag = np.zeros(m), np.zeros(m)
    for b in range(nblk):
        o = order[b * BJ:(b + 1) * BJ]
        rb = np.where(o >= 0, r[np.maximum(o, 0)], 0.0)
        for s in range(BJ):
            if o[s] >= 0:
                p = binv[b, s] * rb                       # (rounded products: gamma_{32 + 1})
                want[o[s]] = math.fsum(p)
                mag[o[s]] = math.fsum(np.abs(p))
    ok = nr.within_bound(zh[:m], want, mag, BJ + 1)
    assert ok.all(), nr.worst(zh[:m], want, mag, BJ + 1)
    assert np.isnan(wsh[nwg])                             # one partial per workgroup, no more
    rz = math.fsum(wsh[:nwg])
    prod = r[:m] * zh[:m]
    assert abs(rz - math.fsum(prod)) <= nr.gamma(m + nwg + 1) * math.fsum(np.abs(prod))


def test_jacobi_diagonal_of_the_canonical_matrix(env):
    """IterativeNormalSolver(precond='jacobi'): dinv = 1 / sum_j a_ij^2 of the matrix with its
    repeated entries summed (not the sum of the squares of the stored pieces)."""
    _hip, dv, torch = env
    from ipsolver.projector import IterativeNormalSolver
    rng = np.random.default_rng(4)
    A = nr.random_csr(rng, 300, 900, rng.integers(1, 12, 300), nr.int_values)
    S = IterativeNormalSolver(dv.DeviceCSR.from_scipy(nr.split_duplicates(A)), precond="jacobi")
    want = 1.0 / np.asarray(A.multiply(A).sum(axis=1)).ravel()
    assert np.array_equal(S.dinv.to_host(), want)


# ----------------------------------------------------------- duplicate Jacobian entries
class _SparseNLP:
    """min 1/2 x'Dx - q'x + 1/4 sum x^4  s.t.  c(x) = J0 x + kappa/2 (J0 o J0)(x o x) - b = 0:
    a Jacobian J0 + kappa (J0 o J0) diag(x) with J0's pattern, random sparsity."""

    def __init__(self, m, n, per, seed, kappa=0.1):
        rng = np.random.default_rng(seed)
        self.J0 = nr.random_csr(rng, m, n, np.full(m, per), lambda r, s: r.standard_normal(s))
        self.W = self.J0.multiply(self.J0).tocsr()
        self.kappa = kappa
        self.d = rng.uniform(1.0, 2.0, n)
        self.q = rng.standard_normal(n)
        xf = rng.uniform(-0.5, 0.5, n)
        self.b = self.J0.dot(xf) + 0.5 * kappa * self.W.dot(xf * xf)
        self.x0 = np.zeros(n)

    def fun(self, x):
        return 0.5 * x.dot(self.d * x) - self.q.dot(x) + 0.25 * np.sum(x ** 4)

    def grad(self, x):
        return self.d * x - self.q + x ** 3

    def hess(self, x):
        return sps.diags(self.d + 3 * x * x, format="csr")

    def cfun(self, x):
        return self.J0.dot(x) + 0.5 * self.kappa * self.W.dot(x * x) - self.b

    def jac(self, x):
        return (self.J0 + self.kappa * self.W.multiply(x[None, :])).tocsr()

    def chess(self, x, v):
        return sps.diags(self.kappa * self.W.T.dot(v), format="csr")


def _solve(ipsolver, fun, x0, grad, hess, cons):
    xs = []

    def record(state):
        xs.append(np.array(state.x, copy=True))
        return False
    res = ipsolver.minimize_constrained(fun, x0, grad, hess, cons, callback=record)
    return res, xs


def _assert_same_run(a, b):
    (ra, xa), (rb, xb) = a, b
    assert (ra.status, ra.niter, ra.cg_niter) == (rb.status, rb.niter, rb.cg_niter)
    assert len(xa) == len(xb) and all(np.array_equal(u, v) for u, v in zip(xa, xb))
    assert np.array_equal(ra.x, rb.x)


def _nonlinear_pair(ipsolver, p, wrap_kind=("equals", 0.0)):
    runs = []
    for dup in (False, True):
        jac = (lambda x: nr.split_duplicates(p.jac(x))) if dup else p.jac
        con = ipsolver.NonlinearConstraint(p.cfun, wrap_kind, jac, p.chess)
        runs.append(_solve(ipsolver, p.fun, p.x0, p.grad, p.hess, con))
    return runs


def test_duplicate_entries_banded_nlp():
    """CenteredBandedNLP (the banded solver: ipx_aat_band_w) with its Jacobian's values stored
    as two halves each: the same iterates, bit for bit, as the canonical Jacobian."""
    import ipsolver
    from ipsolver.synthetic import CenteredBandedNLP
    p = CenteredBandedNLP(2000, 200, seed=3)
    runs = []
    for dup in (False, True):
        jac = (lambda x: nr.split_duplicates(p.constr_jac(x))) if dup else p.constr_jac
        con = ipsolver.NonlinearConstraint(p.constr_fun, ("equals", 0), jac, p.constr_hess)
        runs.append(_solve(ipsolver, p.fun, p.x0, p.grad, p.hess, con))
    assert runs[0][0].niter > 1
    _assert_same_run(*runs)


def test_duplicate_entries_dense_fallback():
    """A random-sparsity Jacobian of 150 rows: A A' is not banded in any order, the dense
    Cholesky of A A' formed by ipx_aat_dense takes it."""
    import ipsolver
    p = _SparseNLP(150, 600, 6, seed=1)
    a, b = _nonlinear_pair(ipsolver, p)
    assert a[0].niter > 1
    _assert_same_run(a, b)


def test_duplicate_entries_iterative(monkeypatch):
    """The same with the dense limit lowered below m (as tests/test_gpu_qp.py does), so the
    block-Jacobi preconditioned CG (ipx_blockjacobi_build) solves with A A'."""
    import ipsolver
    from ipsolver import projector
    from ipsolver.dense import DenseNormalSolver
    monkeypatch.setattr(DenseNormalSolver, "MAX_ROWS_FROM_SPARSE", 100)
    seen = []
    real = projector.IterativeNormalSolver.__init__

    def spy(self, *a, **k):
        seen.append(1)
        return real(self, *a, **k)
    monkeypatch.setattr(projector.IterativeNormalSolver, "__init__", spy)
    p = _SparseNLP(300, 1200, 4, seed=2)
    a, b = _nonlinear_pair(ipsolver, p)
    assert seen, "the iterative normal solver was not used"
    assert a[0].niter > 1
    _assert_same_run(a, b)


def test_duplicate_entries_linear_constraint():
    """A LinearConstraint whose matrix stores its entries twice (the dense fallback)."""
    import ipsolver
    p = _SparseNLP(120, 500, 5, seed=4, kappa=0.0)
    J = p.J0.copy()
    D = nr.split_duplicates(J)
    keep = (D.data.copy(), D.indices.copy(), D.indptr.copy())
    runs = [_solve(ipsolver, p.fun, p.x0, p.grad, p.hess,
                   ipsolver.LinearConstraint(M, ("equals", p.b))) for M in (J, D)]
    assert runs[0][0].niter > 1
    _assert_same_run(*runs)
    assert all(np.array_equal(u, v) for u, v in zip(keep, (D.data, D.indices, D.indptr)))


def test_device_pattern_with_a_repeated_entry_is_refused(env):
    """Device-callback mode: a CSRPattern storing (row, column) twice is a ValueError that names
    the entry -- through with_sorted_indices and through a device `jac`."""
    import torch
    import ipsolver
    _hip, dv, _ = env
    indptr = np.array([0, 2, 4], dtype=np.int32)
    indices = np.array([1, 0, 2, 1], dtype=np.int32)         # row 1: (1, 2), (1, 1) -- fine
    ok = dv.DeviceCSR(dv.CSRPattern(indptr, indices, (2, 3)), torch.ones(4, dtype=torch.float64,
                                                                          device="cuda"))
    assert ok.with_sorted_indices().pattern.indices_h.tolist() == [0, 1, 1, 2]
    bad_idx = np.array([0, 2, 2, 2], dtype=np.int32)         # (1, 2) twice, out of order too
    bad = dv.DeviceCSR(dv.CSRPattern(indptr, np.array([0, 1, 2, 2], dtype=np.int32), (2, 3)),
                       torch.ones(4, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match=r"\(1, 2\)"):
        bad.with_sorted_indices()
    bad2 = dv.DeviceCSR(dv.CSRPattern(indptr, bad_idx, (2, 3)),
                        torch.ones(4, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match=r"\(1, 2\)"):
        bad2.with_sorted_indices()
    vals = torch.tensor([1.0, 0.5, 0.5, 1.0], dtype=torch.float64, device="cuda")
    pat = dv.CSRPattern(indptr, np.array([0, 1, 1, 1], dtype=np.int32), (2, 3))   # (1, 1) twice

    def jac(x):
        return dv.DeviceCSR(pat, vals)
    x0 = torch.zeros(3, dtype=torch.float64, device="cuda")
    con = ipsolver.NonlinearConstraint(lambda x: torch.stack((x[0], x[1] + x[2])) * 0.0,
                                       ("equals", 0.0), jac, None)
    with pytest.raises(ValueError, match=r"\(1, 1\)"):
        ipsolver.minimize_constrained(lambda x: float((x * x).sum().item()), x0,
                                      lambda x: 2 * x, lambda x: torch.full_like(x, 2.0), con)
