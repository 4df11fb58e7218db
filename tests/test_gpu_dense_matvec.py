"""The dense matvec kernels and the K-split Gram path of csrc/dense.hip through the C ABI,
against exact int64 results on integer-valued data, against a longdouble reference within a
derived worst-case bound on real-valued data (tests/primitive_cases.py), and against numpy
models of the summation orders their comments document.  Every operand is a view into a larger
buffer: outputs sit between sentinels that must survive, inputs between NaN and then between
0.0, which must give the same bits."""
import types

import numpy as np
import pytest

import primitive_cases as pc
from primitive_cases import Guarded

pytestmark = pytest.mark.gpu

EINVAL = -1
LD = np.longdouble


@pytest.fixture(scope="module")
def gpu():
    from ipsolver import _hip, device as dv
    return types.SimpleNamespace(hip=_hip, dv=dv, lib=_hip.load(), ws=dv.ctx().ws)


def _ptr(g):
    return None if g is None else g.ptr


def run_gemv(gpu, c, lda, reduce, fill=np.nan, alias=False):
    """(y, red or None) of ipx_dense_gemv on the case's operands: A at an odd double offset with
    leading dimension lda, x / diag / yin / yout at mixed parities."""
    m = c["m"]
    A = Guarded(c["A"], offset=1, fill=fill, lda=lda)
    x = Guarded(c["x"], offset=2, fill=fill)
    diag = Guarded(c["diag"], offset=1, fill=fill) if c["diag"] is not None else None
    if alias:
        yout = yin = Guarded(c["yin"], offset=1)
    else:
        yin = Guarded(c["yin"], offset=3, fill=fill) if c["yin"] is not None else None
        yout = Guarded.output(m, offset=1)
    red = Guarded.output(2, offset=1) if reduce else None
    gpu.hip.call("ipx_dense_gemv", m, c["n"], A.ptr, lda, x.ptr, c["alpha"], _ptr(diag), c["beta"],
                 _ptr(yin), yout.ptr, _ptr(red), gpu.ws.data_ptr() if reduce else None,
                 gpu.dv.stream_ptr())
    for g in (A, x, diag, yin):
        if g is not None and g is not yout:
            g.read()                                            # (inputs: nothing written at all)
            assert pc.same_bits(g.t.cpu().numpy(), g.before)
    return yout.read(), (red.read() if reduce else None)


def _shapes(n):
    return [pc.GEMV_TALL] if n == pc.GEMV_TALL[1] else pc.gemv_shapes(n)


GEMV_PARAMS = pc.GEMV_N + (pc.GEMV_TALL[1],)


@pytest.mark.parametrize("n", GEMV_PARAMS)
def test_gemv_integer_exact(gpu, n):
    """Every epilogue, with and without the reduction, at lda = n, n + 1, n + 7: y, sum y^2 and
    sum x*y (square shapes; 0 otherwise) equal the int64 results."""
    for m, n in _shapes(n):
        for ep in pc.EPILOGUES:
            c = pc.gemv_case(m, n, "int", ep)
            want = pc.gemv_ref(c, np.int64)[0]
            for lda in (n, n + 1, n + 7):
                for reduce in (False, True):
                    y, red = run_gemv(gpu, c, lda, reduce)
                    assert np.array_equal(y, want), (m, n, ep, lda, reduce)
                    if reduce:
                        assert red[0] == pc.sumsq_ref(want, np.int64)[0], (m, n, ep, lda)
                        xy = pc.dot_ref(c["x"], want, np.int64)[0] if m == n else 0
                        assert red[1] == xy, (m, n, ep, lda)


@pytest.mark.parametrize("kind", ["real", "wide"])
@pytest.mark.parametrize("n", GEMV_PARAMS)
def test_gemv_real_bound_and_neighbours(gpu, n, kind):
    """|y - ref| <= (nterms + 4) 2^-53 sum|terms| per output against the longdouble reference,
    the reductions likewise against the longdouble sums of the y the kernel produced; and the
    same bits whether the slack around the inputs (lda > n) holds NaN or 0.0."""
    worst = 0.0
    for m, n in _shapes(n):
        for ep in pc.EPILOGUES:
            c = pc.gemv_case(m, n, kind, ep)
            ref, sumabs, nt = pc.gemv_ref(c, LD)
            reduce = kind == "real"              # (the squares of the wide case overflow)
            y, red = run_gemv(gpu, c, n + 1, reduce, fill=np.nan)
            y0, red0 = run_gemv(gpu, c, n + 1, reduce, fill=0.0)
            assert pc.same_bits(y, y0), (m, n, ep)
            ok, ratio = pc.within(y, ref, nt, sumabs)
            worst = max(worst, ratio)
            assert ok, (m, n, ep, ratio)
            if reduce:
                assert pc.same_bits(red, red0)
                r, sa, k = pc.sumsq_ref(y, LD)
                ok, ratio = pc.within(red[0], r, k, sa)
                assert ok, (m, n, ep, "sum y^2", ratio)
                if m == n:
                    r, sa, k = pc.dot_ref(c["x"], y, LD)
                    ok, ratio = pc.within(red[1], r, k, sa)
                    assert ok, (m, n, ep, "sum x*y", ratio)
                else:
                    assert red[1] == 0.0
    print("gemv %s n=%d: worst |err| / bound = %.3f" % (kind, n, worst))


@pytest.mark.parametrize("n", pc.GEMV_N)
def test_gemv_order_model(gpu, n):
    """The order the results of the dense path are pinned to: lane l sums columns l, l + 64, ...
    left to right, pairwise tree over each row of 16 lanes, (r0 + r1) + (r2 + r3) -- every
    product and sum rounded once.  Bit for bit, in both template forms."""
    for m, n in pc.gemv_shapes(n):
        for ep in pc.EPILOGUES:
            c = pc.gemv_case(m, n, "real", ep, seed=1)
            want = pc.gemv_order_model(c)
            for reduce in (False, True):
                y, _ = run_gemv(gpu, c, n + 7, reduce)
                assert np.array_equal(y, want), (m, n, ep, reduce)


def test_gemv_yin_aliases_yout(gpu):
    """yin == yout is legal (DenseNormalSolver, rmatvec_sub): every row reads its own entry
    before it writes it."""
    for (m, n), ep in (((130, 65), "yin"), ((65, 65), "both"), (pc.GEMV_TALL, "yin")):
        c = pc.gemv_case(m, n, "int", ep)
        y, red = run_gemv(gpu, c, n + 1, True, alias=True)
        want = pc.gemv_ref(c, np.int64)[0]
        assert np.array_equal(y, want)
        assert red[0] == pc.sumsq_ref(want, np.int64)[0]


def test_gemv_no_rows(gpu):
    c = pc.gemv_case(0, 5, "int", "none")
    y, red = run_gemv(gpu, c, 5, True)
    assert y.size == 0 and pc.same_bits(red, [0.0, 0.0])


def test_gemv_refuses_diag_on_a_rectangle(gpu):
    """diag_r pairs with x_r: refused (before any launch) unless m == n, like ipx_csr_spmv.
    (x is held long enough for either shape all the same.)"""
    for m, n in ((7, 5), (5, 7)):
        rng = np.random.default_rng(m)
        A, x = Guarded(pc.ints(rng, (m, n))), Guarded(pc.ints(rng, max(m, n)))
        diag, yout = Guarded(pc.ints(rng, m)), Guarded.output(m)
        before = gpu.lib.ipx_launch_count()
        rc = gpu.lib.ipx_dense_gemv(m, n, A.ptr, n, x.ptr, 1.0, diag.ptr, 0.0, None, yout.ptr,
                                    None, None, gpu.dv.stream_ptr())
        assert rc == EINVAL and gpu.lib.ipx_launch_count() == before
        assert np.array_equal(yout.read().view(np.uint64), np.full(m, pc.SENTINEL))


# ---------------------------------------------------------------- gemvt
def run_gemvt(gpu, c, ldb, fill=np.nan):
    B = Guarded(c["B"], offset=1, fill=fill, lda=ldb)
    x = Guarded(c["x"], offset=1, fill=fill)
    y = Guarded.output(c["n"], offset=1)
    gpu.hip.call("ipx_dense_gemvt", c["m"], c["n"], B.ptr, ldb, x.ptr, y.ptr, gpu.dv.stream_ptr())
    return y.read()


@pytest.mark.parametrize("n", pc.GEMVT_N)
def test_gemvt_integer_exact(gpu, n):
    """The 16-row unrolled body and the 4-row tail of every wave, ldb > n; no rows: zeros."""
    for m in pc.GEMVT_M:
        c = pc.gemvt_case(m, n, "int")
        want = pc.gemvt_ref(c, np.int64)[0]
        for ldb in (n + 1, n + 7):
            assert np.array_equal(run_gemvt(gpu, c, ldb), want), (m, n, ldb)
        if m == 0:
            assert pc.same_bits(run_gemvt(gpu, c, n + 1), np.zeros(n))


@pytest.mark.parametrize("kind", ["real", "wide"])
@pytest.mark.parametrize("n", pc.GEMVT_N)
def test_gemvt_real_bound_and_neighbours(gpu, n, kind):
    worst = 0.0
    for m in pc.GEMVT_M:
        c = pc.gemvt_case(m, n, kind)
        ref, sumabs, nt = pc.gemvt_ref(c, LD)
        y, y0 = run_gemvt(gpu, c, n + 3, np.nan), run_gemvt(gpu, c, n + 3, 0.0)
        assert pc.same_bits(y, y0), (m, n)
        ok, ratio = pc.within(y, ref, nt, sumabs)
        worst = max(worst, ratio)
        assert ok, (m, n, ratio)
    print("gemvt %s n=%d: worst |err| / bound = %.3f" % (kind, n, worst))


@pytest.mark.parametrize("n", pc.GEMVT_N)
def test_gemvt_order_model(gpu, n):
    """Wave g sums rows g, g + 4, ... in order; ((p0 + p1) + p2) + p3.  Bit for bit."""
    for m in pc.GEMVT_M:
        c = pc.gemvt_case(m, n, "real", seed=1)
        assert np.array_equal(run_gemvt(gpu, c, n + 1), pc.gemvt_order_model(c)), (m, n)


# ---------------------------------------------------------------- Gram with K splits
def run_gram(gpu, A_h, lda, off, splits, fill=np.nan):
    m, n = A_h.shape
    M = int(gpu.lib.ipx_dense_padded(m))
    A = Guarded(A_h, offset=off, fill=fill, lda=lda)
    G = Guarded.output((M, M), offset=1)
    nws = int(gpu.lib.ipx_gram_ws_doubles(m, splits))
    assert (nws == 0) == (splits <= 1)
    ws = Guarded.output(nws, offset=0) if nws else None
    gpu.hip.call("ipx_gram_f64_mfma_split", m, n, A.ptr, lda, G.ptr, _ptr(ws), splits,
                 gpu.dv.stream_ptr())
    if ws is not None:
        ws.read()                                               # (its slack untouched)
    assert pc.same_bits(A.t.cpu().numpy(), A.before)
    return G.read()


def _padding_is_identity(G, m):
    want = np.eye(len(G))
    want[:m, :m] = G[:m, :m]
    return pc.same_bits(G, want)


@pytest.mark.parametrize("m,n,lda,off", pc.GRAM_SHAPES)
def test_gram_splits_integer_exact(gpu, m, n, lda, off):
    """ipx_gram_f64_mfma_split with 2, 3 and 8 splits (fewer K-chunks than splits: empty
    splits; uneven ranges) on integer data: every entry exact, G = G' bit for bit, identity in
    the padding, the bits of the one-split result."""
    A = pc.gram_case(m, n, "int")
    want = pc.gram_ref(A, np.int64)[0]
    G1 = run_gram(gpu, A, lda, off, 1)
    assert np.array_equal(G1[:m, :m], want) and _padding_is_identity(G1, m)
    for splits in pc.GRAM_SPLITS:
        G = run_gram(gpu, A, lda, off, splits)
        assert np.array_equal(G[:m, :m], want), splits
        assert pc.same_bits(G, G.T) and _padding_is_identity(G, m), splits
        assert pc.same_bits(G, G1), splits


@pytest.mark.parametrize("m,n,lda,off", pc.GRAM_SHAPES)
def test_gram_splits_real_bound_and_neighbours(gpu, m, n, lda, off):
    """(n + splits) 2^-53 sum_k |a_ik||a_jk| per entry; the same bits with NaN and with 0.0 in
    the slack between the rows of A (lda > n) and around it."""
    A = pc.gram_case(m, n, "real")
    ref, sumabs, nt = pc.gram_ref(A, LD)
    worst = 0.0
    for splits in (1,) + pc.GRAM_SPLITS:
        G = run_gram(gpu, A, lda, off, splits, np.nan)
        assert pc.same_bits(G, run_gram(gpu, A, lda, off, splits, 0.0)), splits
        ok, ratio = pc.within(G[:m, :m], ref, nt, sumabs, slack=splits)
        worst = max(worst, ratio)
        assert ok, (splits, ratio)
        assert pc.same_bits(G, G.T) and _padding_is_identity(G, m), splits
    print("gram %dx%d: worst |err| / bound = %.3f" % (m, n, worst))


def test_gram_split_choice_is_self_consistent(gpu):
    """ipx_gram_splits returns 1..8 and more than 1 only with >= 16 K-chunks per split;
    ipx_gram_ws_doubles is 0 for splits <= 1 and splits x tiles x 64 x 64 otherwise."""
    lib = gpu.lib
    for m, n in ((3, 8), (70, 100), (130, 1001), (500, 4096), (2000, 6000), (2016, 512),
                 (513, 2050), (64, 511), (64, 512), (64, 1024)):
        s = int(lib.ipx_gram_splits(m, n))
        assert 1 <= s <= 8
        assert s == 1 or ((n + 31) // 32) // s >= 16, (m, n, s)
        assert (int(lib.ipx_gram_ws_doubles(m, s)) == 0) == (s <= 1)
        nt = int(lib.ipx_dense_padded(m)) // 64
        for k in (0, 1):
            assert int(lib.ipx_gram_ws_doubles(m, k)) == 0
        for k in (2, 3, 8):
            assert int(lib.ipx_gram_ws_doubles(m, k)) == k * (nt * (nt + 1) // 2) * 64 * 64
