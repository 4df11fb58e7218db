"""The radius test of the fused projected-CG loop formed from carried sums
(csrc/cg.hip, ipx_cg_args.xsums): k_cg_step2_hp leaves sum x^2, sum x p, sum p^2 of the x and p
it has just formed, the next iteration's k_cg_step1_ar reads neither vector and the test of
qp_subproblem.py:583 uses ||x + alpha p||^2 = XX + 2 alpha XP + alpha^2 PP.

Only the decision variable differs from the form that reads x and p (debug form
``read-xn2``), so whole runs must agree with it BIT FOR BIT: iterates, iteration counts,
exits.  Inside a relative band of 1e-9 around the radius, or with sums whose tag is not the
iteration's, the device decides nothing (stop code 10) and the host forms the norm.

Sizes: (50000, 5000) has 74 row tiles of H -- two 64-entry slices of partials for the fused
step1 to fold, the second one partial, the last row tile short; (2000, 200) has three row
tiles and one slice.  Both are below the resident kernel's range limit, hence ``no-resident``.
"""
import functools

import numpy as np
import pytest
import torch

from banded_setup import BandedInstance
from conftest import host

pytestmark = pytest.mark.gpu
SHAPES = [(50000, 5000), (2000, 200)]
CARRIED, READING = "no-resident", "no-resident,read-xn2"


@functools.lru_cache(maxsize=None)
def setup(n, m):
    """Instance, device operators and projections of one shape, built once for the module."""
    import ipsolver.device as dv
    import ipsolver.projector as proj
    inst = BandedInstance(n, m)
    A = dv.DeviceCSR.from_scipy(inst.A)
    H = dv.DeviceCSR.from_scipy(inst.H)
    Z, _, Y = proj.projections(A)
    return inst, A, H, Z, Y


def solve(monkeypatch, form, n, m, c=None, **kw):
    """One projected_cg call under a debug form: (x, info, change of STATS, the loop object)."""
    import ipsolver.qp as qp
    import ipsolver.cg_fused as cg_fused
    inst, A, H, Z, Y = setup(n, m)
    monkeypatch.setenv("IPX_DEBUG_FORMS", form)
    before = dict(cg_fused.STATS)
    x, info = qp.projected_cg(H, inst.c if c is None else c, Z, Y, np.zeros(m), **kw)
    delta = {k: cg_fused.STATS[k] - before[k] for k in before}
    L = next(reversed(cg_fused._POOL.values()))          # parked there by the call
    assert delta["calls"] == 1 and delta["resident_calls"] == 0
    # the run stayed on the two fused kernels, and took the form it was asked for
    assert L.args.A_span > 0 and L.args.H_hmax > 0
    assert bool(L.args.xsums) == (form == CARRIED)
    return host(x), info, delta, L


def both(monkeypatch, n, m, **kw):
    xc, ic, dc, _ = solve(monkeypatch, CARRIED, n, m, **kw)
    xr, ir, dr, _ = solve(monkeypatch, READING, n, m, **kw)
    assert dr["radius_undecided"] == 0
    assert ic == ir, (ic, ir)
    assert np.array_equal(xc, xr)
    return xc, ic, dc


_NORMS = {}


def free_norms(monkeypatch, n, m, k):
    """||x_k|| and ||x_(k-1)|| after k and k - 1 iterations without a radius, and ||x|| at the
    minimiser; computed once per shape (reading form) and shared."""
    import ipsolver.qp as qp
    if (n, m, k) not in _NORMS:
        inst, A, H, Z, Y = setup(n, m)
        monkeypatch.setenv("IPX_DEBUG_FORMS", READING)
        xk, info = qp.projected_cg(H, inst.c, Z, Y, np.zeros(m), tol=0, max_iter=k)
        xj, _ = qp.projected_cg(H, inst.c, Z, Y, np.zeros(m), tol=0, max_iter=k - 1)
        x_free, _ = qp.projected_cg(H, inst.c, Z, Y, np.zeros(m), tol=1e-12)
        assert info["niter"] == k
        _NORMS[n, m, k] = (float(np.linalg.norm(host(xk))), float(np.linalg.norm(host(x_free))),
                           float(np.linalg.norm(host(xj))))
    return _NORMS[n, m, k]


@pytest.mark.parametrize("n,m", SHAPES)
def test_radius_never_reached(monkeypatch, n, m):
    """trust_radius = 1e300 (the benchmark's): 40 iterations in batches of 4, 8, 16, 12 -- the
    first iteration reads x and p, every other one is carried, across the batch boundaries
    too -- and no test is left to the host."""
    x, info, d = both(monkeypatch, n, m, trust_radius=1e300, tol=0, max_iter=40)
    assert info["niter"] == 40 and info["stop_cond"] == 1
    assert d["radius_undecided"] == 0 and d["batches"] == 4
    nt = setup(n, m)[2].pattern.ntiles
    assert (nt > 64) == (n == 50000)


@pytest.mark.parametrize("where", ["half", "late"])
@pytest.mark.parametrize("n,m", SHAPES)
def test_radius_crossed(monkeypatch, n, m, where):
    """half: trust_radius = 0.5 ||x_free|| (crossed early).  late: a radius midway between
    ||x_5|| and ||x_6|| -- the iterates of CG grow in norm, so the sixth iteration crosses it,
    one whose test is formed from the carried sums, in the call's second batch."""
    rho6, rfree, rho5 = free_norms(monkeypatch, n, m, 6)
    if where == "half":
        kw = dict(trust_radius=0.5 * rfree)
    else:
        kw = dict(trust_radius=0.5 * (rho5 + rho6), tol=0, max_iter=40)
    x, info, d = both(monkeypatch, n, m, **kw)
    assert info["stop_cond"] == 2 and info["hits_boundary"]
    if where == "late":
        assert rho5 < rho6 and info["niter"] == 6
    assert d["radius_undecided"] == 0


@pytest.mark.parametrize("n,m", SHAPES)
def test_band_goes_to_the_host(monkeypatch, n, m):
    """A radius 1e-11 (relative) either side of ||x_6||: inside the band of 1e-9, and 1e4
    rounding errors (5e-15, the spread of two summation orders) away from a tie, so every
    direct sum decides the same way.  The device leaves exactly that one test to the host;
    the two radii end on opposite sides, each as the reading form does."""
    k = 6
    rho = free_norms(monkeypatch, n, m, k)[0]
    x_hi, i_hi, d_hi = both(monkeypatch, n, m, trust_radius=rho * (1 + 1e-11), tol=0, max_iter=40)
    x_lo, i_lo, d_lo = both(monkeypatch, n, m, trust_radius=rho * (1 - 1e-11), tol=0, max_iter=40)
    assert d_hi["radius_undecided"] == 1 and d_lo["radius_undecided"] == 1
    # below ||x_6||: iteration 6 leaves the ball; above: it stays inside and a later one leaves
    assert (i_lo["niter"], i_lo["stop_cond"], i_lo["hits_boundary"]) == (k, 2, True)
    assert i_hi["niter"] > k and i_hi["stop_cond"] == 2


def test_pooled_loop_object(monkeypatch):
    """Two calls through one pooled loop object (same patterns, other c and radius): no tag
    of the first call's sums survives into the second."""
    import ipsolver.cg_fused as cg_fused
    n, m = SHAPES[0]
    inst = setup(n, m)[0]
    rfree = free_norms(monkeypatch, n, m, 6)[1]
    c2 = inst.c * np.linspace(0.5, 1.5, n)
    calls = [dict(trust_radius=0.5 * rfree, tol=0, max_iter=40),
             dict(c=c2, trust_radius=1e300, tol=0, max_iter=9)]
    out = {}
    for form in (CARRIED, READING):
        reused = cg_fused.POOL_STATS["reused"]
        out[form] = [solve(monkeypatch, form, n, m, **kw) for kw in calls]
        assert cg_fused.POOL_STATS["reused"] >= reused + 1
        assert out[form][0][3] is out[form][1][3]            # the same loop object
    for (xc, ic, dc, _), (xr, ir, _, _) in zip(out[CARRIED], out[READING]):
        assert ic == ir and np.array_equal(xc, xr) and dc["radius_undecided"] == 0
    assert out[CARRIED][0][1]["stop_cond"] == 2 and out[CARRIED][1][1]["niter"] == 9


def test_refinement_every_iteration(monkeypatch):
    """orth_tol = 1e-30: every iteration stops for the refinement of projections.py:72-78 and
    is finished by ipx_cg_resume, which changes x and p outside the fused kernel -- the batch
    after it must read them again."""
    n, m = SHAPES[0]
    P = setup(n, m)[3].projector
    saved = P.orth_tol
    P.orth_tol = 1e-30
    try:
        x, info, d = both(monkeypatch, n, m, trust_radius=1e300, tol=0, max_iter=6)
    finally:
        P.orth_tol = saved
    assert d["refine_events"] > 0 and d["radius_undecided"] == 0
    assert info["niter"] == 6


def test_batch_continuation_without_the_flag(monkeypatch):
    """The benchmark's own pattern on a bare loop object: prime, iterate(0, 7), iterate(7, 12)
    without xsums_carry -- iteration 7 reads x and p -- against one iterate(0, 12), where it is
    carried.  And with a tag that is not the iteration's, the device decides nothing."""
    import ipsolver.cg_fused as cg_fused
    import ipsolver.device as dv
    from ipsolver import _hip
    n, m = SHAPES[0]
    inst, A, H, Z, Y = setup(n, m)
    monkeypatch.setenv("IPX_DEBUG_FORMS", CARRIED)
    lib, st, P = _hip.load(), dv.stream_ptr(), Z.projector
    x0 = Y.dot(-dv.DVec.zeros(m))
    r0 = Z.dot(H.dot(x0) + dv.DVec.from_host(inst.c))
    g0 = Z.dot(r0)
    L = cg_fused._Loop(H, P, None, None)
    assert L.args.xsums and L.args.A_span > 0 and L.args.H_hmax > 0 and not L.args.resident
    init = np.zeros(L.state.numel())
    init[cg_fused.ST_RTG0] = g0.sumsq_amax()[0]
    init[cg_fused.ST_RADIUS] = 1e300
    init[cg_fused.ST_ORTH_RHS] = P.orth_tol * P.norm_A
    init = torch.from_numpy(init).to(L.state.device)

    def prime():
        L.x.copy_(x0.t)
        L.r.copy_(r0.t)
        _hip.call("ipx_axpby", n, -1.0, dv._p(g0.t), 0.0, None, dv._p(L.p), st)
        L.state.copy_(init)
        _hip.check(lib.ipx_cg_hp(L.ref(), st), "ipx_cg_hp")

    def run(*batches):
        prime()
        for a, b in batches:
            _hip.check(lib.ipx_cg_iterate(L.ref(), a, b, st), "ipx_cg_iterate")
        s = L.state.tolist()
        return L.x.cpu().numpy().copy(), int(s[cg_fused.ST_STOP]), int(s[cg_fused.ST_IT_DONE])

    nt = H.pattern.ntiles
    x_one, stop, done = run((0, 12))
    assert (stop, done) == (0, 12)
    assert L.xsums[3 * nt].item() == 12.0                   # the tag the last iteration left
    x_two, stop, done = run((0, 7), (7, 12))
    assert (stop, done) == (0, 12)
    assert np.array_equal(x_one, x_two)
    # the caller's flag on a batch that does NOT continue the one before: the tag (7) is not
    # the iteration's (9), stop code 10 and nothing committed
    prime()
    _hip.check(lib.ipx_cg_iterate(L.ref(), 0, 7, st), "ipx_cg_iterate")
    x7 = L.x.cpu().numpy().copy()
    L.args.xsums_carry = 1
    _hip.check(lib.ipx_cg_iterate(L.ref(), 9, 12, st), "ipx_cg_iterate")
    L.args.xsums_carry = 0
    s = L.state.tolist()
    assert (int(s[cg_fused.ST_STOP]), int(s[cg_fused.ST_IT_DONE])) == (10, 7)
    assert np.array_equal(L.x.cpu().numpy(), x7)
