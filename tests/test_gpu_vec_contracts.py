"""The vector primitives of csrc/vec.hip against the numpy expression each one stands for:
bit for bit on ordinary data at sizes around the block / grid boundaries and at view offsets 0
and 1, exactly on integer data for the reductions, and on special values -- NaN, +-inf, -0.0,
the smallest subnormal, 1.797e308 at the first, an interior and the last position.  Outputs
are views between sentinels that must survive; the kernels that switch between 16-byte and
8-byte accesses by pointer parity (k_axpby2, k_gather_rows) run at every parity combination,
with NaN and then 0.0 around their inputs.

sum_log: the accuracy of the device's double-precision ``log`` is not taken from a document
here; the sum is compared with the sum of longdouble logarithms within
(n + 2) 2^-53 sum|log s_i| plus one ulp (2^-52 |log s_i|) per term, and the observed fraction
of that margin is printed (0.13 at most on the MI355X, at n = 2)."""
import itertools
import math
import types

import numpy as np
import pytest

import primitive_cases as pc
from primitive_cases import Guarded

pytestmark = pytest.mark.gpu

LD = np.longdouble


@pytest.fixture(scope="module")
def gpu():
    from ipsolver import _hip, device as dv, backend_hip as bh
    return types.SimpleNamespace(hip=_hip, dv=dv, bh=bh, lib=_hip.load(), ws=dv.ctx().ws)


def call(gpu, name, *args):
    gpu.hip.call(name, *args, gpu.dv.stream_ptr())


def _i32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


class Ops:
    """Every elementwise primitive on host arrays: operands as views at double offset ``off``
    (NaN around them), the result out of a sentinel-guarded view."""

    def __init__(self, gpu, off):
        self.gpu, self.off = gpu, off

    def _in(self, a):
        return Guarded(a, offset=self.off, fill=np.nan)

    def _map(self, name, n, *args):
        out = Guarded.output(n, offset=self.off)
        call(self.gpu, name, n, *[a.ptr if isinstance(a, Guarded) else a for a in args], out.ptr)
        return out.read()

    def fill(self, n, v):
        return self._map("ipx_fill", n, float(v))

    def affine(self, a, x, b):
        return self._map("ipx_affine", len(x), float(a), self._in(x), float(b))

    def mul(self, x, y):
        return self._map("ipx_mul", len(x), self._in(x), self._in(y))

    def clip(self, x, lb, ub):
        return self._map("ipx_clip", len(x), self._in(x), self._in(lb), self._in(ub))

    def maximum(self, x, c):
        return self._map("ipx_max_scalar", len(x), self._in(x), float(c))

    def where_positive(self, v, a, c):
        return self._map("ipx_where_positive", len(v), self._in(v), self._in(a), float(c))

    def gather(self, x, idx, sign=None, shift=None):
        idx_d = _i32(idx)
        return self._map("ipx_gather", len(idx), self._in(x), idx_d.data_ptr(),
                         None if sign is None else self._in(sign),
                         None if shift is None else self._in(shift))

    def scatter(self, name, x, idx, base):
        idx_d, xg = _i32(idx), self._in(x)
        out = Guarded(base, offset=self.off)
        call(self.gpu, name, len(idx), xg.ptr, idx_d.data_ptr(), out.ptr)
        return out.read()

    def assign_negated_where(self, s, mask, c):
        sg, mg, cg = Guarded(s, offset=self.off), self._in(mask), self._in(c)
        call(self.gpu, "ipx_assign_negated_where", len(s), sg.ptr, mg.ptr, cg.ptr)
        return sg.read()

    def reduce(self, name, n, k, *arrays):
        """The first k outputs of a two-launch reduction over views of ``arrays``."""
        gs = [self._in(a) for a in arrays]
        out = Guarded.output(k, offset=1)
        call(self.gpu, name, n, *[g.ptr for g in gs], out.ptr, self.gpu.ws.data_ptr())
        return out.read()


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", pc.VEC_N)
def test_elementwise_primitives(gpu, n, off):
    """fill, affine, mul, clip, maximum, where_positive, gather (sign / shift / repeated
    indices), scatter into a pre-filled array, scatter_add over a permutation,
    assign_negated_where: the bits of the numpy expression."""
    rng = np.random.default_rng([n, off])
    op = Ops(gpu, off)
    x, y, z = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    assert pc.same_bits(op.fill(n, -2.5), np.full(n, -2.5))
    assert pc.same_bits(op.affine(-1.5, x, 0.3), -1.5 * x + 0.3)
    assert pc.same_bits(op.mul(x, y), x * y)
    lb, ub = np.minimum(y, z), np.maximum(y, z)
    assert pc.same_bits(op.clip(x, lb, ub), np.minimum(np.maximum(x, lb), ub))
    assert pc.same_bits(op.maximum(x, 0.125), np.maximum(x, 0.125))
    assert pc.same_bits(op.where_positive(x, y, -7.0), np.where(x > 0, y, -7.0))
    # gather: n outputs out of a source of another length, indices repeat
    src = rng.standard_normal(n // 2 + 3)
    idx = rng.integers(0, len(src), n)
    sign, shift = rng.choice([-1.0, 1.0], n), rng.standard_normal(n)
    assert pc.same_bits(op.gather(src, idx), src[idx])
    assert pc.same_bits(op.gather(src, idx, sign=sign), sign * src[idx])
    assert pc.same_bits(op.gather(src, idx, shift=shift), src[idx] - shift)
    assert pc.same_bits(op.gather(src, idx, sign, shift), sign * (src[idx] - shift))
    # scatter: some of the entries of a pre-filled array, the others keep their bits
    base = rng.standard_normal(n + 4)
    where = rng.permutation(n + 4)[:n // 2 + 1]
    want = base.copy()
    want[where] = x[:len(where)]
    assert pc.same_bits(op.scatter("ipx_scatter", x[:len(where)], where, base), want)
    perm = rng.permutation(n)
    want = y.copy()
    want[perm] += x
    assert pc.same_bits(op.scatter("ipx_scatter_add", x, perm, y), want)
    mask = (rng.random(n) < 0.4).astype(np.float64)
    want = x.copy()
    want[mask != 0] = -y[mask != 0]
    assert pc.same_bits(op.assign_negated_where(x, mask, y), want)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", pc.VEC_N)
def test_reductions_exact_on_integers(gpu, n, off):
    """dot and the sum of squares of integer data are exact in any order; max |x| and the count
    of coordinates outside a box are exact on any data.  Through the two-launch entries and
    through the package's folded reads."""
    op = Ops(gpu, off)
    x, y = pc.vec_ints(n, 1), pc.vec_ints(n, 2)
    xi, yi = x.astype(np.int64), y.astype(np.int64)
    assert op.reduce("ipx_dot", n, 1, x, y)[0] == (xi * yi).sum()
    nr = op.reduce("ipx_norms", n, 2, x)
    assert nr[0] == (xi * xi).sum() and nr[1] == np.abs(xi).max()
    lb, ub = np.minimum(y, 0.0) - 100.0, np.maximum(y, 0.0) + 100.0
    outside = np.count_nonzero(~((lb <= x) & (x <= ub)))
    assert op.reduce("ipx_box_inside", n, 1, x, lb, ub)[0] == outside
    dv = gpu.dv
    gx, gy, gl, gu = (Guarded(a, offset=off, fill=np.nan) for a in (x, y, lb, ub))
    X, Y = dv.DVec(gx.tensor()), dv.DVec(gy.tensor())
    assert X.dot(Y) == (xi * yi).sum()
    assert X.sumsq_amax() == [float((xi * xi).sum()), float(np.abs(xi).max())]
    assert dv.count_outside_box(X, dv.DVec(gl.tensor()), dv.DVec(gu.tensor())) == outside
    r = np.random.default_rng(n).standard_normal(n)
    assert op.reduce("ipx_norms", n, 2, r)[1] == np.abs(r).max()


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", pc.VEC_N)
def test_sum_log(gpu, n, off):
    """out[0] = sum of log over the positive entries, out[1] = the number of the others; the
    wrapper's verdict is -inf as soon as one entry is not positive."""
    rng = np.random.default_rng([n, off, 9])
    op = Ops(gpu, off)
    s = np.exp(rng.uniform(-30.0, 30.0, n))
    logs = np.log(s.astype(LD))
    ref, S = logs.sum(), np.abs(logs).sum()
    margin = (n + 2) * LD(pc.U) * S + 2 * LD(pc.U) * S
    got = op.reduce("ipx_sum_log", n, 2, s)
    frac = float(abs(LD(got[0]) - ref) / margin)
    print("sum_log n=%d off=%d: |err| / margin = %.4f" % (n, off, frac))
    assert frac <= 1.0 and got[1] == 0.0
    assert abs(got[0] - math.fsum(np.log(s))) <= float(margin)
    gs = Guarded(s, offset=off, fill=np.nan)
    assert gpu.bh.sum_log(gpu.dv.DVec(gs.tensor())) == got[0]
    # some entries not positive: counted, left out of the sum, verdict -inf
    bad = pc.special_positions(n)
    t = s.copy()
    t[bad] = [0.0, -1.0, -0.0][:len(bad)]
    keep = np.ones(n, dtype=bool)
    keep[bad] = False
    got = op.reduce("ipx_sum_log", n, 2, t)
    assert got[1] == len(bad)
    assert abs(LD(got[0]) - logs[keep].sum()) <= margin
    gt = Guarded(t, offset=off, fill=np.nan)
    assert gpu.bh.sum_log(gpu.dv.DVec(gt.tensor())) == -np.inf


# ---------------------------------------------------------------- special values
def _cmp(value):
    """Bits (signed zeros included) -- values where a NaN is involved (its payload and sign are
    not part of any contract)."""
    return pc.same_values if np.isnan(value) else pc.same_bits


def _norms_every_way(gpu, x):
    """(norm, norm_inf) of a host vector by the folded read, by a ScalarPack, and by both of
    them with a full partial arena (the two-launch reductions)."""
    dv = gpu.dv
    g = Guarded(x, offset=1, fill=0.0)
    X = dv.DVec(g.tensor())
    out = []
    for full in (False, True):
        c = dv.ctx()
        if full:
            c.parts_used = dv.PARTS_ARENA
        out.append((dv.norm(X), dv.norm_inf(X)))
        pk = dv.ScalarPack()
        h = [pk.norm(X), pk.norm_inf(X), pk.sumsq(X)]
        v = pk.read()
        assert c.parts_used == 0
        out.append((v[h[0]], v[h[1]]))
        assert v[h[2]] == X.sumsq_amax()[0] or np.isnan(v[h[2]])
    return out


@pytest.mark.parametrize("value", pc.SPECIALS, ids=lambda v: repr(float(v)))
@pytest.mark.parametrize("n", [3, 1025])
def test_special_values(gpu, n, value):
    """Each primitive on data holding ``value`` at the first, an interior and the last
    position, against its numpy expression."""
    rng = np.random.default_rng([n, 17])
    op = Ops(gpu, 1)
    cmp = _cmp(value)
    plain = rng.standard_normal(n)
    x = pc.with_special(plain, value)
    y, z = rng.standard_normal(n), rng.standard_normal(n)
    lb, ub = np.minimum(y, z), np.maximum(y, z)
    inf = np.full(n, np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        # clip = np.minimum(np.maximum(x, lb), ub): the value in x, in lb, in ub; infinite bounds
        for a, lo, hi in ((x, lb, ub), (x, -inf, inf), (x, -inf, ub), (x, lb, inf),
                          (plain, pc.with_special(lb, value), inf),
                          (plain, -inf, pc.with_special(ub, value))):
            assert pc.same_values(op.clip(a, lo, hi), np.minimum(np.maximum(a, lo), hi))
        assert pc.same_values(op.maximum(x, 0.125), np.maximum(x, 0.125))
        assert pc.same_values(op.maximum(plain, value), np.maximum(plain, value))
        assert pc.same_values(op.maximum(x, 0.0), np.maximum(x, 0.0))
        # where_positive passes bits through
        assert pc.same_bits(op.where_positive(x, y, -7.0), np.where(x > 0, y, -7.0))
        assert pc.same_bits(op.where_positive(y, x, value), np.where(y > 0, x, value))
        # signed zeros (and everything else that is not a NaN) bit for bit
        assert cmp(op.mul(x, y), x * y)
        assert cmp(op.affine(-1.5, x, 0.0), -1.5 * x + 0.0)
        assert cmp(op.affine(1.0, x, value), 1.0 * x + value)
        idx = rng.integers(0, n, n)
        idx[:3] = pc.special_positions(n)
        sign, shift = rng.choice([-1.0, 1.0], n), np.zeros(n)
        assert pc.same_bits(op.gather(x, idx), x[idx])
        assert cmp(op.gather(x, idx, sign, shift), sign * (x[idx] - shift))
        mask = np.ones(n)
        mask[1::2] = 0.0
        want = y.copy()
        want[mask != 0] = -x[mask != 0]
        assert cmp(op.assign_negated_where(y, mask, x), want)
        want = x.copy()
        want[mask != 0] = -y[mask != 0]
        assert cmp(op.assign_negated_where(x, mask, y), want)
        # NaN counts as outside the box
        outside = np.count_nonzero(~((lb <= x) & (x <= ub)))
        assert op.reduce("ipx_box_inside", n, 1, x, lb, ub)[0] == outside
        lbs = pc.with_special(lb, value)
        assert op.reduce("ipx_box_inside", n, 1, plain, lbs, ub)[0] == \
            np.count_nonzero(~((lbs <= plain) & (plain <= ub)))
        # norm(x) and norm(x, inf)
        want2, wantinf = np.sqrt(np.sum(x * x)), np.max(np.abs(x))
        for got2, gotinf in _norms_every_way(gpu, x):
            assert pc.same_values(gotinf, wantinf), (gotinf, wantinf)
            if np.isfinite(want2):
                assert abs(got2 - want2) <= 1e-14 * want2
            else:
                assert pc.same_values(got2, want2), (got2, want2)
        # sum(log s_i if s_i > 0 else -inf) (tr_interior_point.py:93)
        s = pc.with_special(np.exp(plain), value)
        want = math.fsum(math.log(v) if v > 0 else -np.inf for v in s)
        gs = Guarded(s, offset=1, fill=0.0)
        got = gpu.bh.sum_log(gpu.dv.DVec(gs.tensor()))
        if np.isfinite(want):
            assert abs(got - want) <= 1e-13 * sum(abs(math.log(v)) for v in s)
        else:
            assert got == want


# ---------------------------------------------------------------- pointer-parity forms
@pytest.mark.parametrize("n", [2, 256, 1026, 4100])
def test_axpby_every_parity(gpu, n):
    """k_axpby2 (16-byte accesses) runs only when n is even and x, y and out are all 16-byte
    aligned: every parity combination, with and without y, gives a * x + b * y bit for bit,
    writes nothing beside out, and reads nothing beside x and y."""
    rng = np.random.default_rng(n)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    for ox, oy, oo in itertools.product((0, 1), repeat=3):
        for b in (0.0, 0.3):
            want = 2.5 * x + b * y if b else 2.5 * x
            res = []
            for fill in (np.nan, 0.0):
                gx, gy = Guarded(x, offset=ox, fill=fill), Guarded(y, offset=oy, fill=fill)
                out = Guarded.output(n, offset=oo)
                call(gpu, "ipx_axpby", n, 2.5, gx.ptr, b, gy.ptr, out.ptr)
                res.append(out.read())
            assert pc.same_bits(res[0], want) and pc.same_bits(res[1], want), (ox, oy, oo, b)


@pytest.mark.parametrize("ncols", [1, 2, 7, 64, 513, 1030])
def test_gather_rows_every_parity(gpu, ncols):
    """k_gather_rows takes 16-byte accesses where a source row and its destination share their
    16-byte phase (one element peeled when both start on an odd double) and 8-byte ones
    otherwise: even and odd leading dimensions, bases and column offsets -- the block lands where
    it should, its neighbours (between the rows, before and behind) keep their bits, and the
    source's neighbours are not read."""
    rng = np.random.default_rng(ncols)
    rows, src_rows = 9, 6
    idx = rng.integers(0, src_rows, rows)
    sign = rng.choice([-1.0, 1.0], rows)
    out_rows = rows + 2
    dst = rng.permutation(out_rows)[:rows]
    src = rng.standard_normal((src_rows, ncols))
    idx_d, dst_d = _i32(idx), _i32(dst)
    for os_, lds_extra, oo, ldo_extra, col0 in itertools.product((0, 1), (0, 1, 2), (0, 1),
                                                                 (0, 1), (0, 1, 2)):
        lds, width = ncols + lds_extra, col0 + ncols + 1
        ldo = width + ldo_extra
        base = rng.standard_normal((out_rows, width))
        want = base.copy()
        want[dst, col0:col0 + ncols] = sign[:, None] * src[idx]
        res = []
        for fill in (np.nan, 0.0):
            gs = Guarded(src, offset=os_, fill=fill, lda=lds)
            sg = Guarded(sign, offset=1, fill=fill)
            out = Guarded(base, offset=oo, lda=ldo)
            call(gpu, "ipx_dense_gather_rows", rows, ncols, gs.ptr, lds, idx_d.data_ptr(), sg.ptr,
                 dst_d.data_ptr(), out.ptr, ldo, col0)
            res.append(out.read())
        assert pc.same_bits(res[0], want) and pc.same_bits(res[1], want), \
            (os_, lds, oo, ldo, col0)
