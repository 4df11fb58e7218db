"""The fused epilogue of the CSR product (csrc/spmv.hip): all eight template forms
(diag, yin, reduce) on all three tile branches -- short rows staged in LDS, tiles of more rows
than the fast path takes, one row longer than a tile -- through ipx_csr_spmv, and the extended
entry ipx_csr_spmv_ex (explicit row vector, device guard, unfolded partials) with ipx_fold2.

One integer-valued matrix of 3000 rows (tests/primitive_cases.py spmv_matrix: empty rows, a
run of 1100 empty rows that fills a tile by its row count, one row of 2198 entries) makes y,
sum y^2 and sum xrow*y exact in any order; its real-valued twin holds the existing contract
(short rows sum left to right like scipy's csr_matvec, bit for bit) and the derived bound on the
long row.

The branch for tiles of more than IPX_SPMV_TILE_ROWS (1024) rows is reached with a tile table
from ipx_csr_tiles_host itself, asked for up to 2048 rows per tile (the run of empty rows then
shares one tile with its neighbours); the package's own tables never ask for more than 1024."""
import itertools
import types

import numpy as np
import pytest

import primitive_cases as pc
from primitive_cases import Guarded

pytestmark = pytest.mark.gpu

EINVAL = -1
LD = np.longdouble
TILE_ROWS = 1024                    # IPX_SPMV_TILE_ROWS
FORMS = list(itertools.product((False, True), repeat=3))        # (diag, yin, reduce)


@pytest.fixture(scope="module")
def gpu():
    from ipsolver import _hip, device as dv
    return types.SimpleNamespace(hip=_hip, dv=dv, lib=_hip.load(), ws=dv.ctx().ws)


class Problem:
    """A matrix on the device with its operands (uploaded once, never written)."""

    def __init__(self, gpu, kind, shape, max_rows):
        import torch
        self.kind, self.shape = kind, shape
        self.M = M = pc.spmv_matrix(kind, *shape)
        self.ops = pc.spmv_operands(kind, *shape)
        self.tiles_h = gpu.dv._tiles_for(M.indptr, _tile_nnz(gpu), max_rows)
        self.ntiles = len(self.tiles_h) // 2 - 1
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.rowptr, self.colidx = dev(M.indptr.astype(np.int32)), dev(M.indices.astype(np.int32))
        self.val, self.tiles = dev(M.data), dev(self.tiles_h)
        self.d = {k: Guarded(self.ops[k], offset=1 + i % 2, fill=np.nan)
                  for i, k in enumerate(("x", "xrow", "diag", "yin"))}
        self.long = np.diff(M.indptr) > _tile_nnz(gpu)
        rows = np.diff(self.tiles_h[:self.ntiles + 1])
        self.max_tile_rows = int(rows.max())

    def head(self, alpha=None):
        p = lambda t: t.data_ptr()
        return (self.shape[0], self.shape[1], p(self.rowptr), p(self.colidx), p(self.val),
                p(self.tiles), self.ntiles, self.d["x"].ptr,
                self.ops["alpha"] if alpha is None else alpha)

    def tail(self, has_diag, has_yin):
        return (self.d["diag"].ptr if has_diag else None, self.ops["beta"] if has_yin else 0.0,
                self.d["yin"].ptr if has_yin else None)


def _tile_nnz(gpu):
    return gpu.hip.SPMV_TILE_NNZ


_PROBLEMS = {}


def problem(gpu, kind, shape=(3000, 3000), max_rows=TILE_ROWS):
    key = (kind, shape, max_rows)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = Problem(gpu, kind, shape, max_rows)
    return _PROBLEMS[key]


def run_spmv(gpu, P, has_diag, has_yin, reduce, alpha=None):
    yout, red = Guarded.output(P.shape[0], offset=1), Guarded.output(2, offset=1)
    square = 1 if P.shape[0] == P.shape[1] else 0
    rc = gpu.lib.ipx_csr_spmv(*P.head(alpha), *P.tail(has_diag, has_yin), yout.ptr, square,
                              red.ptr if reduce else None, gpu.ws.data_ptr(), gpu.dv.stream_ptr())
    return rc, yout.read(), red.read()


def run_spmv_ex(gpu, P, has_diag, has_yin, xrow, guard_value):
    """(rc, y, partials, folded red) of ipx_csr_spmv_ex + ipx_fold2."""
    import torch
    yout = Guarded.output(P.shape[0], offset=1)
    part, red = Guarded.output(2 * P.ntiles, offset=1), Guarded.output(2, offset=1)
    guard = torch.full((1,), float(guard_value), dtype=torch.float64, device="cuda")
    st = gpu.dv.stream_ptr()
    rc = gpu.lib.ipx_csr_spmv_ex(*P.head(), *P.tail(has_diag, has_yin), yout.ptr,
                                 None if xrow is None else xrow.ptr, part.ptr, guard.data_ptr(),
                                 st)
    gpu.hip.call("ipx_fold2", part.ptr, P.ntiles, red.ptr, None, st)
    return rc, yout.read(), part.read(), red.read()


def check_form(P, y, red, has_diag, has_yin, reduce, xrow_h):
    """y and red of one launch against the int64 results (integer data), or the row-order
    model bit for bit on the short rows and the derived bound on the long one (real data)."""
    M, ops = P.M, P.ops
    what = (P.kind, has_diag, has_yin, reduce)
    xr = xrow_h if xrow_h is not None else np.zeros(P.shape[0])
    if P.kind == "int":
        want = pc.spmv_ref(M, ops, has_diag, has_yin, xr, np.int64)[0]
        assert np.array_equal(y, want), what
        if reduce:
            assert red[0] == pc.sumsq_ref(want, np.int64)[0], what
            assert red[1] == (pc.dot_ref(xr, want, np.int64)[0] if xrow_h is not None else 0), what
        return
    ref, sumabs, nt = pc.spmv_ref(M, ops, has_diag, has_yin, xr, LD)
    ok, ratio = pc.within(y, ref, nt, sumabs)
    assert ok, what + (ratio,)
    model = ops["alpha"] * M.dot(ops["x"])                      # scipy: left to right
    if has_diag:
        model = model + ops["diag"] * xr
    if has_yin:
        model = model + ops["beta"] * ops["yin"]
    assert np.array_equal(y[~P.long], model[~P.long]), what
    if reduce:
        r, sa, k = pc.sumsq_ref(y, LD)
        assert pc.within(red[0], r, k, sa)[0], what
        if xrow_h is not None:
            r, sa, k = pc.dot_ref(xr, y, LD)
            assert pc.within(red[1], r, k, sa)[0], what
        else:
            assert red[1] == 0.0


@pytest.mark.parametrize("max_rows", [TILE_ROWS, 2 * TILE_ROWS])
@pytest.mark.parametrize("kind", ["int", "real"])
def test_spmv_all_forms_square(gpu, kind, max_rows):
    """The eight forms on the square matrix; max_rows = 2048 puts the run of empty rows into a
    tile of more than 1024 rows (the generic-loop branch)."""
    P = problem(gpu, kind, max_rows=max_rows)
    assert P.long.sum() == 1
    assert (P.max_tile_rows == TILE_ROWS) if max_rows == TILE_ROWS else (P.max_tile_rows > TILE_ROWS)
    for has_diag, has_yin, reduce in FORMS:
        rc, y, red = run_spmv(gpu, P, has_diag, has_yin, reduce)
        assert rc == 0
        check_form(P, y, red, has_diag, has_yin, reduce, P.ops["x"])
        if not reduce:
            assert np.array_equal(red.view(np.uint64), np.full(2, pc.SENTINEL))


def test_spmv_plain_rows_equal_scipy(gpu):
    """The existing contract on this matrix: without an epilogue the short rows are scipy's."""
    P = problem(gpu, "real")
    rc, y, _ = run_spmv(gpu, P, False, False, False, alpha=1.0)
    assert rc == 0 and np.array_equal(y[~P.long], P.M.dot(P.ops["x"])[~P.long])


@pytest.mark.parametrize("kind", ["int", "real"])
def test_spmv_rectangular(gpu, kind):
    """No row vector: the forms without diag run (sum xrow*y = 0), diag is refused."""
    P = problem(gpu, kind, shape=(3000, 4000))
    for has_diag, has_yin, reduce in FORMS:
        rc, y, red = run_spmv(gpu, P, has_diag, has_yin, reduce)
        if has_diag:
            assert rc == EINVAL
            assert np.array_equal(y.view(np.uint64), np.full(len(y), pc.SENTINEL))
            continue
        assert rc == 0
        check_form(P, y, red, False, has_yin, reduce, None)


@pytest.mark.parametrize("shape", [(3000, 3000), (3000, 4000)])
@pytest.mark.parametrize("kind", ["int", "real"])
def test_spmv_ex_row_vector_partials_and_guard(gpu, kind, shape):
    """ipx_csr_spmv_ex with a row vector of its own (diag * xrow, sum xrow * y -- also for a
    rectangular matrix), its unfolded partials folded by ipx_fold2; against ipx_csr_spmv bit for
    bit where the two compute the same; a non-zero guard leaves yout and the partials alone."""
    P = problem(gpu, kind, shape=shape)
    xrow, xrow_h = P.d["xrow"], P.ops["xrow"]
    for has_diag, has_yin in itertools.product((False, True), repeat=2):
        rc, y, part, red = run_spmv_ex(gpu, P, has_diag, has_yin, xrow, 0.0)
        assert rc == 0
        check_form(P, y, red, has_diag, has_yin, True, xrow_h)
        if not has_diag:
            # the same y as the plain entry, so the same sum y^2 -- folded in the same order
            rc2, y2, red2 = run_spmv(gpu, P, False, has_yin, True)
            assert rc2 == 0 and pc.same_bits(y, y2) and red[0] == red2[0]
    if shape[0] == shape[1]:
        # a second buffer holding x's values: everything the plain entry computes, bit for bit
        xcopy = Guarded(P.ops["x"], offset=2, fill=0.0)
        for has_diag, has_yin in itertools.product((False, True), repeat=2):
            rc, y, part, red = run_spmv_ex(gpu, P, has_diag, has_yin, xcopy, 0.0)
            rc2, y2, red2 = run_spmv(gpu, P, has_diag, has_yin, True)
            assert rc == 0 and rc2 == 0
            assert pc.same_bits(y, y2) and pc.same_bits(red, red2)
    else:
        rc, y, part, red = run_spmv_ex(gpu, P, True, False, None, 0.0)
        assert rc == EINVAL                                   # diag without any row vector
    # guard set: nothing is written (the fold then sums the sentinels: not looked at)
    rc, y, part, _ = run_spmv_ex(gpu, P, True, True, xrow, 1.0)
    assert rc == 0
    assert np.array_equal(y.view(np.uint64), np.full(len(y), pc.SENTINEL))
    assert np.array_equal(part.view(np.uint64), np.full(len(part), pc.SENTINEL))
