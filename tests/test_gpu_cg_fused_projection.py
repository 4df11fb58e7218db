"""The projection half of a projected-CG iteration as ONE launch (csrc/banded.hip
k_step1_solve_tail: step1, w = A r_next, the cyclic-reduction solve, g = r_next - A'v on the
solve's windows) against the three launches it shortens to two.

Every sum of the fused launch is formed in the order of the launches it replaces, so the two
forms must agree BIT FOR BIT: iterates, residuals, partials, the state block, the stops.  Only
part2 (the ||x + alpha p||^2 partials: one per solve workgroup instead of one per row tile of A)
is laid out differently; it feeds a comparison alone.

Inside a batch the roles of r and r_next alternate; whatever the iteration count or stop code,
``a->r`` must hold the current residual when an entry point returns (odd counts, split batches).

Shapes (rows per solve workgroup: 260): (2000, 200) one workgroup, its window cut at both
matrix edges; (5200, 520) exactly two full workgroups; (5210, 521) a third workgroup that owns
one row; (50000, 5000) 20 workgroups, the last partial, 74 row tiles of H, two carried slices.
All are below the resident kernel's limit, where the fused projection is not the default: it is
forced (``fused_projection=True``) on the separate launches (``no-resident``).
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sps
import torch

from banded_setup import BandedInstance

pytestmark = pytest.mark.gpu
SHAPES = [(2000, 200), (5200, 520), (5210, 521), (50000, 5000)]
_TINY = 1e-25


class Problem:
    """Device operators, projections and the host-primed start (x0 = 0, r0 = Z c, g0 = Z r0) of
    one instance: computed once and shared, never written to."""

    def __init__(self, A, H, c):
        import ipsolver.device as dv
        import ipsolver.projector as proj
        self.n, self.m = A.shape[1], A.shape[0]
        self.A = dv.DeviceCSR.from_scipy(A)
        self.H = dv.DeviceCSR.from_scipy(H)
        self.Z, _, self.Y = proj.projections(self.A)
        self.P = self.Z.projector
        self.c = dv.DVec.from_host(c)
        self.r0 = self.Z.dot(self.c)
        self.g0 = self.Z.dot(self.r0)
        self.rt_g = self.g0.sumsq_amax()[0]
        self.gnorm = float(dv.norm(self.r0))
        torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def problem(n, m, variant="plain"):
    inst = BandedInstance(n, m)
    A, H = inst.A.tocsr(), inst.H.tocsr()
    if variant == "negative":
        # one negative diagonal entry, far below the rest of the spectrum: p'Hp <= 0 early
        H = (H - sps.csr_matrix(([1e6], ([n // 2], [n // 2])), shape=H.shape)).tocsr()
        H.sort_indices()
    if variant == "short-row":
        # one row of A with 14 entries instead of 15: not every row has one length
        A = A.tolil()
        row = m // 2
        A[row, A.rows[row][7]] = 0.0
        A = A.tocsr()
        A.eliminate_zeros()
        A.sort_indices()
        assert sorted(set(np.diff(A.indptr))) == [14, 15]
    return Problem(A, H, inst.c)


def loop(monkeypatch, q, fused, read_xn2=False):
    import ipsolver.cg_fused as cg_fused
    monkeypatch.setenv("IPX_DEBUG_FORMS", "no-resident,read-xn2" if read_xn2 else "no-resident")
    L = cg_fused._Loop(q.H, q.P, None, None, resident=False, fused_projection=fused)
    assert not L.args.resident and L.args.A_span > 0 and L.args.H_hmax > 0 and L.args.At_qv > 0
    assert bool(L.args.xsums) == (not read_xn2)
    return L


def bound(L):
    a = L.args
    return a.fused_proj == 1 and bool(a.A_ell_val) and bool(a.A_ell_off16) and bool(a.r_where) \
        and bool(a.P_win) and bool(a.A_rowfirst) and 1 <= a.A_rl <= 16 and 0 < a.P_nspan <= 4096


def prime(L, q, radius=1e300, tol=0.0):
    """bench.py's priming: device copies and one H.p, no host synchronisation."""
    import ipsolver.cg_fused as cg_fused
    import ipsolver.device as dv
    from ipsolver import _hip
    st = dv.stream_ptr()
    L.args.no_radius = 1 if np.isinf(radius) else 0
    L.x.zero_()
    L.r.copy_(q.r0.t)
    _hip.call("ipx_axpby", q.n, -1.0, dv._p(q.g0.t), 0.0, None, dv._p(L.p), st)
    init = np.zeros(L.state.numel())
    init[cg_fused.ST_RTG0] = q.rt_g
    init[cg_fused.ST_TOL] = tol
    init[cg_fused.ST_RADIUS] = radius
    init[cg_fused.ST_ORTH_RHS] = q.P.orth_tol * q.P.norm_A
    L.state.copy_(torch.from_numpy(init))
    _hip.check(_hip.load().ipx_cg_hp(L.ref(), st), "ipx_cg_hp")


def iterate(L, *batches):
    import ipsolver.device as dv
    from ipsolver import _hip
    lib, st = _hip.load(), dv.stream_ptr()
    it = 0
    for k in batches:
        _hip.check(lib.ipx_cg_iterate(L.ref(), it, it + k, st), "ipx_cg_iterate")
        it += k
    torch.cuda.synchronize()


def launches_per_iteration(L):
    """As tests/test_gpu_cg_launch_plan.py counts them: with stop code 9 every kernel returns at
    once; (launches of six iterations - launches of one) / 5."""
    import ipsolver.cg_fused as cg_fused
    import ipsolver.device as dv
    from ipsolver import _hip
    lib, st = _hip.load(), dv.stream_ptr()
    saved = L.state.clone()
    L.state[cg_fused.ST_STOP] = 9.0
    counts = []
    for k in (1, 6):
        before = int(lib.ipx_launch_count())
        _hip.check(lib.ipx_cg_iterate(L.ref(), 0, k, st), "ipx_cg_iterate")
        counts.append(int(lib.ipx_launch_count()) - before)
    torch.cuda.synchronize()
    L.state.copy_(saved)
    assert (counts[1] - counts[0]) % 5 == 0
    return (counts[1] - counts[0]) // 5


FIELDS = ("x", "p", "r", "Hp", "part3", "part4", "state")


def assert_same(Lf, L3, fields=FIELDS):
    for name in fields:
        assert torch.equal(getattr(Lf, name), getattr(L3, name)), name


@pytest.mark.parametrize("n,m", SHAPES)
def test_tables_stay_inside_the_spans(monkeypatch, n, m):
    """The index tables of the fused launch, on the host: every column a window row reaches and
    every own variable lies inside the workgroup's span, the span inside the kernel's LDS, the
    ELL-transposed copy holds A's entries in their CSR order."""
    import ipsolver.cg_fused as cg_fused
    q = problem(n, m)
    L = loop(monkeypatch, q, True)
    assert bound(L)
    a = L.args
    rl, rows_wg, nwg = int(a.A_rl), L.geometry[1], L.geometry[2]
    H = 1 << L.pcr_L
    assert rows_wg + 2 * H <= 512
    win = L.fp_tabs[3].cpu().numpy().astype(np.int64).reshape(nwg, 2)
    first = L.fp_tabs[1].cpu().numpy().astype(np.int64)
    off = L.A_ell_off16.cpu().numpy().view(np.uint16).astype(np.int64).reshape(rl, m)
    vown = L.vown.cpu().numpy().astype(np.int64)
    pat = q.A.pattern
    cols = pat.indices_h.astype(np.int64).reshape(m, rl)
    assert np.array_equal(first[None, :] + off, cols.T)
    assert np.all(win[:, 0] >= 0) and np.all(win[:, 1] <= n) and np.all(win[:, 1] > win[:, 0])
    assert int(np.max(win[:, 1] - win[:, 0])) == a.P_nspan <= 4096
    for b in range(nwg):
        lo, hi = max(b * rows_wg - H, 0), min((b + 1) * rows_wg + H, m)
        assert cols[lo:hi].min() >= win[b, 0] and cols[lo:hi].max() < win[b, 1]
        assert win[b, 0] <= vown[b] and vown[b + 1] <= win[b, 1]
    assert vown[0] == 0 and vown[-1] == n
    torch.cuda.synchronize()
    val = L.A_ell_val.cpu().numpy().reshape(rl, m)
    assert np.array_equal(val, q.A.val.cpu().numpy().reshape(m, rl).T)
    assert launches_per_iteration(L) == 2
    assert launches_per_iteration(loop(monkeypatch, q, False)) == 3


@pytest.mark.parametrize("mode", ["carried", "inf", "read-xn2"])
@pytest.mark.parametrize("n,m", SHAPES)
def test_form_against_form(monkeypatch, n, m, mode):
    """40 iterations with tol = 0 from the same primed state: trust_radius = 1e300 with the
    carried sums, +inf, and 1e300 with x and p read in every iteration."""
    q = problem(n, m)
    radius = np.inf if mode == "inf" else 1e300
    out = []
    for fused in (True, False):
        L = loop(monkeypatch, q, fused, read_xn2=mode == "read-xn2")
        assert bound(L) == fused
        prime(L, q, radius)
        iterate(L, 40)
        out.append(L)
    Lf, L3 = out
    import ipsolver.cg_fused as cg_fused
    s = Lf.state.tolist()
    assert int(s[cg_fused.ST_STOP]) == 0 and int(s[cg_fused.ST_IT_DONE]) == 40
    assert_same(Lf, L3)


@pytest.mark.parametrize("batches", [(1,), (7,), (1, 6), (3, 4), (1, 1)])
@pytest.mark.parametrize("n,m", SHAPES)
def test_r_is_settled_after_every_call(monkeypatch, n, m, batches):
    """Odd iteration counts in one ipx_cg_iterate call and in two: the current r is in a->r when
    the call returns."""
    q = problem(n, m)
    out = []
    for fused in (True, False):
        L = loop(monkeypatch, q, fused)
        prime(L, q)
        iterate(L, *batches)
        out.append(L)
    assert_same(*out)


def _stop_case(monkeypatch, q, radius, tol):
    import ipsolver.cg_fused as cg_fused
    res = []
    for fused in (True, False):
        L = loop(monkeypatch, q, fused)
        assert bound(L) == fused
        prime(L, q, radius, tol)
        iterate(L, 40)
        s = L.state.tolist()
        res.append((int(s[cg_fused.ST_STOP]), int(s[cg_fused.ST_NITER]), L))
    (cf, nf, Lf), (c3, n3, L3) = res
    assert (cf, nf) == (c3, n3)
    assert torch.equal(Lf.x, L3.x)
    # ... and everything else the host's exit paths read (ST_XNORM2, written at a radius stop,
    # is folded from part2, whose layout differs by design: its last bits may differ)
    assert_same(Lf, L3, ("p", "r", "Hp"))
    sf, s3 = Lf.state.clone(), L3.state.clone()
    sf[cg_fused.ST_XNORM2] = s3[cg_fused.ST_XNORM2] = 0.0
    assert torch.equal(sf, s3)
    return cf, nf


@pytest.mark.parametrize("n,m", SHAPES)
def test_stops(monkeypatch, n, m):
    """The ``ball`` variant of pcg_variants (radius 0.6 ||Z c||), a radius that is crossed, the
    default tolerance and negative curvature: the same stop code, iteration count and x as the
    three launches.  On these instances the minimiser lies at 0.38 ||Z c|| (measured: ||x_40|| =
    4.30 against a radius of 6.73 at (2000, 200), 21.2 against 33.5 at (50000, 5000)), so the
    ``ball`` variant runs its 40 iterations inside the ball in both forms; the radius stop is
    therefore asserted on half the norm of the free run's x_40, which the iterates of CG, growing
    in norm, must cross."""
    import ipsolver.cg_fused as cg_fused
    q = problem(n, m)
    kw = BandedInstance.pcg_variants(q, q.gnorm)
    code, niter = _stop_case(monkeypatch, q, kw["ball"]["trust_radius"], 0.0)
    assert code in (0, 2) and niter >= 1
    L = loop(monkeypatch, q, False)
    prime(L, q)
    iterate(L, 40)
    assert int(L.state[cg_fused.ST_STOP].item()) == 0
    half = 0.5 * float(torch.linalg.vector_norm(L.x).item())
    code, niter = _stop_case(monkeypatch, q, half, 0.0)
    assert code == 2 and 1 <= niter < 40
    # default_tol: qp_subproblem.py:529-542 (code 4)
    tol = max(min(0.01 * np.sqrt(q.rt_g), 0.1 * q.rt_g), _TINY)
    code, niter = _stop_case(monkeypatch, q, 1e300, tol)
    assert code == 4 and 1 <= niter < 40
    # negative curvature (code 3)
    qn = problem(n, m, "negative")
    code, niter = _stop_case(monkeypatch, qn, 1e300, 0.0)
    assert code == 3


@pytest.mark.parametrize("n,m", SHAPES)
def test_a_stopped_launch_stores_nothing(monkeypatch, n, m):
    import ipsolver.cg_fused as cg_fused
    q = problem(n, m)
    L = loop(monkeypatch, q, True)
    prime(L, q)
    L.state[cg_fused.ST_STOP] = 9.0
    for name, fill in (("r_next", 3.0), ("v", 5.0), ("part2", 7.0), ("part3", 11.0), ("part4", 13.0)):
        getattr(L, name).fill_(fill)
    before = {k: getattr(L, k).clone() for k in ("r", "r_next", "v", "part2", "part3", "part4",
                                                  "xsums", "x", "p", "Hp", "state")}
    iterate(L, 3)
    for k, v in before.items():
        assert torch.equal(getattr(L, k), v), k


@pytest.mark.parametrize("b_zero,steps", [(True, 0), (True, 1), (False, 0)])
def test_priming(monkeypatch, b_zero, steps):
    """ipx_cg_prime with and without the fused projection, b zero (with and without the
    projections' correction steps armed) and b random: the two projections are one launch each
    instead of the A x product + the solve with its tail -- two launches less -- and leave the
    same bits."""
    import ipsolver.device as dv
    from ipsolver import _hip
    n, m = 5210, 521
    q = problem(n, m)
    rng = np.random.default_rng(11)
    b = None if b_zero else dv.DVec.from_host(rng.standard_normal(m))
    out, counts = [], []
    lib = _hip.load()
    for fused in (True, False):
        L = loop(monkeypatch, q, fused)
        assert bound(L) == fused
        for name in ("x", "p", "r", "Hp"):
            getattr(L, name).zero_()
        ctx_ = dv.ctx()
        ctx_.out.zero_()
        pat = q.A.pattern
        b_rows = None if b is None else q.P.rows_in(b)
        before = int(lib.ipx_launch_count())
        _hip.call("ipx_cg_prime", L.ref(), dv._p(pat.tiles), pat.ntiles, dv._p(q.c.t),
                  None if b_rows is None else dv._p(b_rows.t), dv._p(ctx_.out), dv._p(ctx_.ws),
                  0.0, 1e300, float(q.P.orth_tol), float(q.P.norm_A), float(q.P.CANCELLATION),
                  0, steps, dv.stream_ptr())
        counts.append(int(lib.ipx_launch_count()) - before)
        torch.cuda.synchronize()
        out.append((L, ctx_.out[:14].clone()))
    assert counts[0] == counts[1] - 2
    (Lf, redf), (L3, red3) = out
    assert torch.equal(redf, red3)
    assert_same(Lf, L3, ("x", "r", "p", "Hp", "state"))


def test_rows_of_two_lengths_fall_back(monkeypatch):
    """A Jacobian with one row of 14 entries: the three launches, unchanged results."""
    n, m = 5210, 521
    q = problem(n, m, "short-row")
    out = []
    for fused in (True, False):
        L = loop(monkeypatch, q, fused)
        assert not bound(L) and L.args.fused_proj == 0
        assert launches_per_iteration(L) == 3
        prime(L, q)
        iterate(L, 7)
        out.append(L)
    assert_same(*out)


# ---- beyond the resident kernel's size: the default, the long p'Hp fold, the sharded loop -------
BIG = (1100000, 110000)      # 424 solve workgroups (> 224), 1619 row tiles of H (> 6 x 256)


def test_default_and_long_fold(monkeypatch):
    """At a size the resident launch cannot hold, the fused projection is the default (debug
    form ``no-fused-projection`` switches it off), and with more than 1536 row tiles of H the
    p'Hp fold takes its strided tail on both forms: the same bits."""
    import ipsolver.cg_fused as cg_fused
    n, m = BIG
    q = problem(n, m)
    monkeypatch.setenv("IPX_DEBUG_FORMS", "no-fused-projection")
    L3 = cg_fused._Loop(q.H, q.P, None, None)
    monkeypatch.delenv("IPX_DEBUG_FORMS")
    Lf = cg_fused._Loop(q.H, q.P, None, None)
    assert Lf.geometry[2] > cg_fused.resident_limits()["max_wg"] and Lf.args.H_ntiles > 1536
    assert bound(Lf) and not bound(L3) and not Lf.args.resident and not L3.args.resident
    assert launches_per_iteration(Lf) == 2 and launches_per_iteration(L3) == 3
    for L in (Lf, L3):
        prime(L, q)
        iterate(L, 5)
    assert int(Lf.state[cg_fused.ST_IT_DONE].item()) == 5
    assert_same(Lf, L3)


def test_pooled_calls_arm_the_form_where_it_pays(monkeypatch):
    """The public call on a pooled loop object: with the same Jacobian object the copy of A is
    current and the form is on whatever the call's length; with new values (a new DeviceCSR on
    the same pattern, as every outer iteration makes one) a short call stays on the three
    launches and makes no copy, a call of FUSED_MIN_BATCH iterations or more makes it.  Same x
    either way."""
    import ipsolver.cg_fused as cg_fused
    import ipsolver.device as dv
    import ipsolver.projector as proj
    import ipsolver.qp as qp
    n, m = BIG
    q = problem(n, m)
    monkeypatch.delenv("IPX_DEBUG_FORMS", raising=False)
    b = np.zeros(m)

    def call(Z, Y, max_iter):
        x, info = qp.projected_cg(q.H, q.c, Z, Y, b, trust_radius=1e300, tol=0, max_iter=max_iter)
        L = next(reversed(cg_fused._POOL.values()))
        return x.t.clone(), info, L

    x20o, info20o, L = call(q.Z, q.Y, 20)
    assert L.fp_tabs is not None and L.args.fused_proj == 1          # (long enough: copy made)
    x6, info6, L1 = call(q.Z, q.Y, 6)
    assert L1 is L and L.args.fused_proj == 1                        # (the copy is current)
    A2 = dv.DeviceCSR(q.A.pattern, q.A.val.clone())
    Z2, _, Y2 = proj.projections(A2)
    x6n, info6n, L2 = call(Z2, Y2, 6)
    assert L2 is L and L.args.fused_proj == 0 and getattr(A2, "_ipx_ellt_done", None) is None
    assert info6n == info6 and torch.equal(x6n, x6)
    x20, info20, L3 = call(Z2, Y2, 20)
    assert L3 is L and L.args.fused_proj == 1 and A2._ipx_ellt_done is not None
    assert info20 == info20o and torch.equal(x20, x20o)


def test_sharded_rank_local_loop_keeps_three_launches(monkeypatch):
    """The row-sharded loop's rank-local block at a size beyond the resident kernel's: no fused
    projection (its partials follow the solve's workgroups, not the rank's own ranges), the
    three launches per iteration, and the solve runs and agrees with one GPU's."""
    import ipsolver.cg_fused as cg_fused
    import ipsolver.qp as qp
    from ipsolver import sharded
    n, m = BIG
    q = problem(n, m)
    monkeypatch.delenv("IPX_DEBUG_FORMS", raising=False)
    inst = BandedInstance(n, m)
    A = inst.A.tocsr()
    lay = sharded.ShardLayout(A.indptr, A.indices, A.shape, 1, 0)
    sh = sharded.Sharding(lay, sharded.ShardComm(), sharded.HipOps())
    As, Hs = sharded.ShardCSR.from_global(sh, inst.A), sharded.ShardHessian.from_global(sh, inst.H)
    Z, _, Y = sharded.projections(As)
    built = []
    real = cg_fused._Loop

    class Recording(real):
        def __init__(self, *args, **kw):
            super().__init__(*args, **kw)
            built.append(self)

    monkeypatch.setattr(cg_fused, "_Loop", Recording)
    calls = sharded.STATS["fused_calls"]
    x, info = qp.projected_cg(Hs, sh.from_global(inst.c, "col"), Z, Y, sh.zeros("row"),
                              trust_radius=1e300, tol=0, max_iter=6)
    monkeypatch.setattr(cg_fused, "_Loop", real)
    assert sharded.STATS["fused_calls"] == calls + 1 and built
    L = built[-1]
    assert L.geometry[2] > cg_fused.resident_limits()["max_wg"]
    assert L.args.fused_proj == 0 and L.fp_tabs is None and not L.args.A_ell_val
    assert info["niter"] == 6
    x1, info1 = qp.projected_cg(q.H, q.c, q.Z, q.Y, np.zeros(m), trust_radius=1e300, tol=0,
                                max_iter=6)
    assert info == info1
    xs, xo = x.to_host(), x1.to_host()
    assert np.max(np.abs(xs - xo)) <= 1e-12 * max(1.0, np.max(np.abs(xo)))
