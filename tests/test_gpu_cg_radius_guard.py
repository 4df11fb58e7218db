"""The radius guard of the fused projected-CG loop (csrc/cg.hip, ipx_cg_args.rguard): with a
finite trust radius the test of qp_subproblem.py:583 is decided from a bound
X + |alpha| Q >= ||x + alpha p|| carried in three device scalars while that bound stays below
the radius -- the loop then runs the kernels of the trust_radius = inf loop.  When the bound
reaches the radius the device stops (code 11), the iteration is finished in the carried-sum form
(ipx_cg_guard_resume) and the call goes on in that form.

The outcome of every test is the exact form's (debug form ``no-radius-guard``), so whole runs
agree with it BIT FOR BIT: iterates, iteration counts, exits.

Shapes: (2000, 200) has three row tiles of H and (50000, 5000) has 74 (two 64-entry slices of the
carried sums), both on the three launches per iteration under ``no-resident``; (5200, 520) runs
the two-launch form with the fused projection forced, as tests/test_gpu_cg_fused_projection.py
forces it.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sps
import torch

from banded_setup import BandedInstance
from conftest import host

pytestmark = pytest.mark.gpu
# (n, m, fused projection)
CASES = [(2000, 200, False), (50000, 5000, False), (5200, 520, True)]
GUARD, EXACT = "no-resident", "no-resident,no-radius-guard"


@pytest.fixture(autouse=True)
def forget_lost_guards():
    """Every test starts with no pattern marked as having lost its guard (ipsolver.cg_fused
    _GUARD_LOST: such patterns start their next calls exact)."""
    import ipsolver.cg_fused as cg_fused
    cg_fused._GUARD_LOST.clear()


@functools.lru_cache(maxsize=None)
def setup(n, m, fused, variant):
    """Instance, device operators and projections of one case, built once for the module (its
    own device objects: the loop pool's signature goes by their patterns)."""
    import ipsolver.device as dv
    import ipsolver.projector as proj
    inst = BandedInstance(n, m)
    Hs = inst.H.tocsr()
    if variant == "ill":
        # D H D with D = 1 .. 1e4: the diagonal entries, which the extreme eigenvalues of a
        # symmetric matrix enclose, spread over >= 1e8
        d = np.logspace(0.0, 4.0, n)
        Hs = (sps.diags(d) @ Hs @ sps.diags(d)).tocsr()
        Hs.sort_indices()
        diag = np.abs(Hs.diagonal())
        assert diag.max() / diag.min() >= 1e8
    A = dv.DeviceCSR.from_scipy(inst.A)
    H = dv.DeviceCSR.from_scipy(Hs)
    Z, _, Y = proj.projections(A)
    return inst, A, H, Z, Y


def solve(monkeypatch, form, case, c=None, variant="plain", watch=None, **kw):
    """One projected_cg call under a debug form: (x, info, change of STATS, the loop object,
    launches of the call, radius_guard as every state read of the call saw it)."""
    import ipsolver.qp as qp
    import ipsolver.cg_fused as cg_fused
    from ipsolver import _hip
    n, m, fused = case
    inst, A, H, Z, Y = setup(n, m, fused, variant)
    monkeypatch.setenv("IPX_DEBUG_FORMS", form)
    if fused:
        real = cg_fused._Loop

        class Forced(real):
            def __init__(self, H, P, lb, ub, **k):
                k.update(resident=False, fused_projection=True)
                real.__init__(self, H, P, lb, ub, **k)

        monkeypatch.setattr(cg_fused, "_Loop", Forced)
        kw.setdefault("batch", 20)          # (long enough for the call to arm the form)
    armed = []

    def seen(L, last):
        armed.append(int(L.args.radius_guard))
        if watch is not None:
            watch(L, last)

    monkeypatch.setattr(cg_fused, "_WATCH_BATCHES", [seen])
    lib = _hip.load()
    before, launches = dict(cg_fused.STATS), int(lib.ipx_launch_count())
    c = inst.c if c is None else c
    if "batch" in kw:
        # (the batch length is the device loop's own argument, below the reference's signature)
        import ipsolver.device as dv
        x, info = cg_fused.projected_cg(H, dv.DVec.from_host(c), Z, Y, dv.DVec.zeros(m),
                                        b_zero=True, **kw)
    else:
        x, info = qp.projected_cg(H, c, Z, Y, np.zeros(m), **kw)
    launches = int(lib.ipx_launch_count()) - launches
    delta = {k: cg_fused.STATS[k] - before[k] for k in before}
    L = next(reversed(cg_fused._POOL.values()))          # parked there by the call
    assert delta["calls"] == 1 and delta["resident_calls"] == 0
    assert L.args.A_span > 0 and L.args.H_hmax > 0 and L.args.xsums and L.args.rguard
    assert L.args.radius_guard == 0                      # a parked block describes the exact form
    if fused and min(kw["batch"], kw.get("max_iter") or n - m) >= 16:
        assert L.args.fused_proj == 1
    if form == EXACT:
        assert not any(armed) and delta["guard_lost"] == 0
    return host(x), info, delta, L, launches, armed


def both(monkeypatch, case, **kw):
    xg, ig, dg, L, lg, armed = solve(monkeypatch, GUARD, case, **kw)
    xe, ie, de, _, le, _ = solve(monkeypatch, EXACT, case, **kw)
    assert ig == ie, (ig, ie)
    assert np.array_equal(xg, xe)
    assert dg["radius_undecided"] == de["radius_undecided"]
    return xg, ig, dg, L, (lg, le), armed


_NORMS = {}


def free_norms(monkeypatch, case, k):
    """||x_k|| and ||x_(k-1)|| after k and k - 1 iterations without a radius, and ||x|| at the
    minimiser; computed once per case (exact form) and shared."""
    if case + (k,) not in _NORMS:
        xk, info = solve(monkeypatch, EXACT, case, tol=0, max_iter=k)[:2]
        xj = solve(monkeypatch, EXACT, case, tol=0, max_iter=k - 1)[0]
        x_free = solve(monkeypatch, EXACT, case, tol=1e-12)[0]
        assert info["niter"] == k
        _NORMS[case + (k,)] = (float(np.linalg.norm(xk)), float(np.linalg.norm(x_free)),
                               float(np.linalg.norm(xj)))
    return _NORMS[case + (k,)]


def launches_per_iteration(L, guard):
    """As tests/test_gpu_cg_launch_plan.py counts them: with stop code 9 every kernel returns at
    once; (launches of six iterations - launches of one) / 5."""
    import ipsolver.cg_fused as cg_fused
    import ipsolver.device as dv
    from ipsolver import _hip
    lib, st = _hip.load(), dv.stream_ptr()
    saved = L.state.clone()
    L.state[cg_fused.ST_STOP] = 9.0
    L.args.radius_guard = 1 if guard else 0
    counts = []
    for k in (1, 6):
        before = int(lib.ipx_launch_count())
        _hip.check(lib.ipx_cg_iterate(L.ref(), 0, k, st), "ipx_cg_iterate")
        counts.append(int(lib.ipx_launch_count()) - before)
    torch.cuda.synchronize()
    L.args.radius_guard = 0
    L.state.copy_(saved)
    assert (counts[1] - counts[0]) % 5 == 0
    return (counts[1] - counts[0]) // 5


@pytest.mark.parametrize("case", CASES)
def test_radius_never_reached(monkeypatch, case):
    """trust_radius = 1e300 (the benchmark's), 40 iterations: the guard holds for the whole
    call, which enqueues what the exact form enqueues -- launch for launch."""
    x, info, d, L, (lg, le), armed = both(monkeypatch, case, trust_radius=1e300, tol=0, max_iter=40)
    assert info["niter"] == 40 and info["stop_cond"] == 1
    assert d["guard_lost"] == 0 and d["radius_undecided"] == 0
    assert armed and all(armed)                  # radius_guard = 1 at every state read
    # (the first call on new device operators builds their cached tables: counted on a repeat)
    x2, info2, _, L2, lg, _ = solve(monkeypatch, GUARD, case, trust_radius=1e300, tol=0, max_iter=40)
    assert L2 is L and info2 == info and np.array_equal(x2, x)
    le = solve(monkeypatch, EXACT, case, trust_radius=1e300, tol=0, max_iter=40)[4]
    assert lg == le, (lg, le)
    per = launches_per_iteration(L, True)
    assert per == launches_per_iteration(L, False) == (2 if case[2] else 3)
    # the bounds the call left: above the norms of its last x and p, and finite
    X, Q, T = L.rguard.tolist()
    assert np.isfinite([X, Q, T]).all() and X == T
    assert X >= np.linalg.norm(x.astype(np.longdouble))


@pytest.mark.parametrize("where", ["half", "late"])
@pytest.mark.parametrize("case", CASES)
def test_radius_crossed(monkeypatch, case, where):
    """half: trust_radius = 0.5 ||x_free||.  late: a radius midway between ||x_5|| and ||x_6||.
    The bound reaches the radius at or before the iteration that crosses it: the guard is lost
    once, on the device, and the carried form decides the rest -- nothing is left to the host."""
    rho6, rfree, rho5 = free_norms(monkeypatch, case, 6)
    if where == "half":
        kw = dict(trust_radius=0.5 * rfree)
    else:
        kw = dict(trust_radius=0.5 * (rho5 + rho6), tol=0, max_iter=40)
    x, info, d, L, _, armed = both(monkeypatch, case, **kw)
    assert info["stop_cond"] == 2 and info["hits_boundary"]
    if where == "late":
        assert rho5 < rho6 and info["niter"] == 6
    assert d["guard_lost"] == 1 and d["radius_undecided"] == 0
    assert armed[0] == 1


def _soundness(monkeypatch, case, variant):
    """batch = 1: X and Q read behind every iteration, against the norms of x and p summed in
    longdouble on the host.  Returns the largest X / ||x|| and Q / ||p|| seen."""
    seen = []

    def watch(L, last):
        X, Q, _ = L.rguard.tolist()
        xs = L.x.cpu().numpy().astype(np.longdouble)
        ps = L.p.cpu().numpy().astype(np.longdouble)
        seen.append((last[1], X, Q, np.sqrt(np.sum(xs * xs)), np.sqrt(np.sum(ps * ps))))

    x, info, d, L, _, armed = solve(monkeypatch, GUARD, case, variant=variant, watch=watch,
                                    trust_radius=1e300, tol=0, max_iter=40, batch=1)
    assert d["guard_lost"] == 0 and all(armed)
    assert len(seen) >= 10, info
    worst_x = worst_p = 1.0
    for it, X, Q, nx, np_ in seen:
        assert np.isfinite(X) and np.isfinite(Q)
        assert X >= nx and Q >= np_, (it, X, float(nx), Q, float(np_))
        if nx > 0:
            worst_x = max(worst_x, float(X / nx))
        if np_ > 0:
            worst_p = max(worst_p, float(Q / np_))
    print("radius guard looseness %s %s: iterations %d  max X/||x|| %.4g  max Q/||p|| %.4g  "
          "last X/||x|| %.4g" % (case, variant, len(seen), worst_x, worst_p,
                                 seen[-1][1] / float(seen[-1][3])))
    return worst_x, worst_p


@pytest.mark.parametrize("case", CASES)
def test_bounds_hold(monkeypatch, case):
    _soundness(monkeypatch, case, "plain")


def test_bounds_hold_ill_conditioned(monkeypatch):
    """An eigenvalue spread >= 1e8: the CG loses orthogonality within the 40 iterations; the
    bounds follow from the triangle inequality alone and hold all the same."""
    _soundness(monkeypatch, CASES[1], "ill")


def test_pooled_loop_object(monkeypatch):
    """Calls through one pooled loop object: the first loses the guard; the second starts exact
    and nothing of the first call's X, Q, T survives; it ends inside the trust region, so the
    third is guarded again."""
    import ipsolver.cg_fused as cg_fused
    case = CASES[1]
    n, m, _ = case
    inst = setup(*case, "plain")[0]
    rfree = free_norms(monkeypatch, case, 6)[1]
    c2 = inst.c * np.linspace(0.5, 1.5, n)
    calls = [dict(trust_radius=0.5 * rfree, tol=0, max_iter=40),
             dict(c=c2, trust_radius=1e300, tol=0, max_iter=9),
             dict(c=c2, trust_radius=1e300, tol=0, max_iter=9)]
    out = {}
    for form in (GUARD, EXACT):
        reused = cg_fused.POOL_STATS["reused"]
        out[form] = []
        for k, kw in enumerate(calls):
            out[form].append(solve(monkeypatch, form, case, **kw))
            L = out[form][-1][3]
            if form == GUARD and k == 1:
                assert not L.rguard.cpu().numpy().any()      # zeroed by the re-binding, not written
        assert cg_fused.POOL_STATS["reused"] >= reused + 2
        assert out[form][0][3] is out[form][1][3] is out[form][2][3]     # the same loop object
    for (xg, ig, dg, *_), (xe, ie, de, *_) in zip(out[GUARD], out[EXACT]):
        assert ig == ie and np.array_equal(xg, xe) and dg["radius_undecided"] == 0
    g = out[GUARD]
    assert g[0][2]["guard_lost"] == 1 and g[0][5][0] == 1
    assert g[1][2]["guard_lost"] == 0 and not any(g[1][5])
    assert g[2][2]["guard_lost"] == 0 and all(g[2][5]) and g[2][5]
    assert g[0][1]["stop_cond"] == 2 and g[1][1]["niter"] == 9


def test_refinement_every_iteration(monkeypatch):
    """orth_tol = 1e-30: every iteration stops for the refinement of projections.py:72-78 and
    is finished by ipx_cg_resume on the vector step2, outside the guard's kernel -- which moves
    the bounds with x and p."""
    case = CASES[1]
    P = setup(*case, "plain")[3].projector
    saved = P.orth_tol
    P.orth_tol = 1e-30
    try:
        x, info, d, L, _, armed = both(monkeypatch, case, trust_radius=1e300, tol=0, max_iter=6)
    finally:
        P.orth_tol = saved
    assert d["refine_events"] > 0 and d["radius_undecided"] == 0 and d["guard_lost"] == 0
    assert info["niter"] == 6 and all(armed)
    X, Q, T = L.rguard.tolist()
    assert X > 0 and X >= np.linalg.norm(x.astype(np.longdouble))
    assert Q >= np.linalg.norm(L.p.cpu().numpy().astype(np.longdouble))
