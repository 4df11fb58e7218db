"""Quasi-Newton Hessians on nonlinear constraints on the GPU: the kernel that forms the pair's
``y`` (``ipx_csr_tdiff_dot``) against the library's host twin, one update through the public
objects against a direct call of ``ipx_lowrank_update``, the callback counts, the form of the
CG loop and ``NonlinearConstraint(hess=LSR1())`` end to end in both callback modes."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sps

import ipsolver
import problems
import constraint_qn_cases as cases
from quasi_newton_twin import CompactTwin
from test_host_logic import run

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b)))


def wide():
    """m = 100, n = 5000, entries in every 37th column: tiles of the transpose reach the row cap
    (1024 rows) long before the nonzero cap, most of their rows empty; several workgroups"""
    m, n = 100, 5000
    cols = np.arange(0, n, 37)
    rows = np.arange(len(cols)) % m
    return cases._pattern(np.concatenate((rows, (rows + 1) % m)), np.concatenate((cols, cols)),
                          m, n)


def band(m=280, n=300):
    ij = [(i, j) for i in range(m) for j in (i, i + 7, i + 20) if j < n]
    return cases._pattern([i for i, _ in ij], [j for _, j in ij], m, n)


GPU_PATTERNS = cases.PATTERNS + [("wide", wide)]


def _device_tdiff(pattern, op, y, base, accumulate):
    import torch
    from ipsolver import quasi_newton as qn
    from ipsolver.device import ctx
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ctx().device)
    qn.tdiff_dot(pattern, t(op["val_new"]), t(op["val_old"]), t(op["v"]), y,
                 base=(t(op["base_new"]), t(op["base_old"])) if base else None,
                 accumulate=accumulate)
    return y


@pytest.mark.parametrize("with_base", [False, True], ids=["nobase", "base"])
@pytest.mark.parametrize("accumulate", [False, True], ids=["set", "accumulate"])
@pytest.mark.parametrize("name,make", GPU_PATTERNS, ids=[n for n, _ in GPU_PATTERNS])
def test_kernel_is_the_host_twin(name, make, accumulate, with_base):
    import torch
    from ipsolver import _hip
    from ipsolver.device import CSRPattern, ctx
    indptr, indices, shape = make()
    pat = CSRPattern(indptr, indices, shape)
    tpat, perm = pat.transpose()
    t_indptr, t_indices, perm_h = cases.transpose(indptr, indices, shape)
    assert np.array_equal(tpat.indptr_h, t_indptr) and np.array_equal(perm.cpu().numpy(), perm_h)
    if name in ("arrow", "wide"):
        assert tpat.ntiles > 1
    assert shape[1] % 256 != 0
    op = cases.operands(shape, len(indices), seed=3 + len(indices))
    y = torch.from_numpy(op["y0"].copy()).to(ctx().device) if accumulate \
        else torch.full((shape[1],), float("nan"), dtype=torch.float64, device=ctx().device)
    _device_tdiff(pat, op, y, with_base, accumulate)
    host_op = dict(op)
    if not with_base:
        host_op["base_new"] = host_op["base_old"] = None
    want = cases.host_twin(_hip.load(), shape, t_indptr, t_indices, perm_h,
                           accumulate=accumulate, **host_op)
    assert np.array_equal(y.cpu().numpy(), want)


def test_kernel_accumulates_two_terms_on_different_patterns():
    import torch
    from ipsolver import _hip
    from ipsolver.device import CSRPattern, ctx
    y = torch.full((300,), float("nan"), dtype=torch.float64, device=ctx().device)
    want = None
    for k, make in enumerate((cases.arrow, band)):
        indptr, indices, shape = make()
        assert shape[1] == 300
        pat = CSRPattern(indptr, indices, shape)
        op = cases.operands(shape, len(indices), seed=11 + k)
        _device_tdiff(pat, op, y, base=k == 0, accumulate=k > 0)
        if k > 0:
            op["base_new"] = op["base_old"] = None
        op["y0"] = want
        want = cases.host_twin(_hip.load(), shape, *cases.transpose(indptr, indices, shape),
                               accumulate=k > 0, **op)
    assert np.array_equal(y.cpu().numpy(), want)


# ---- one update through the public objects --------------------------------------------------
@pytest.mark.parametrize("host_callbacks", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("cls", [ipsolver.LSR1, ipsolver.LBFGS], ids=["lsr1", "lbfgs"])
def test_one_update_through_the_resolver(cls, host_callbacks):
    import torch
    from ipsolver import _hip, quasi_newton as qn
    from ipsolver.device import CSRPattern, DeviceCSR, DVec, ctx, _p, stream_ptr
    indptr, indices, shape = cases.arrow()
    m, n = shape
    assert n == 300
    rng = np.random.default_rng(5)
    x0, x1 = rng.standard_normal(n), rng.standard_normal(n)
    d = rng.uniform(0.5, 4.0, n)
    g0, g1 = d * x0, d * x1                                     # positive curvature: stored
    val0 = rng.standard_normal(len(indices))
    val1 = val0 + 1e-3 * rng.standard_normal(len(indices))
    v0, v1 = rng.standard_normal(m), 0.1 * rng.standard_normal(m)
    strategy = cls(4)
    lagr = qn.LagrangianQN(strategy, n, host_callbacks=host_callbacks)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ctx().device)
    pat = CSRPattern(indptr, indices, shape)
    other = DVec.from_host(np.ones(n))

    def requests(x, g, val, v):
        if host_callbacks:
            J = sps.csr_matrix((val, indices, indptr), shape=shape)
            return x, [qn.QNRequest(n, g=g), other, qn.QNRequest(n, J=J, v=v)]
        return DVec.from_host(x), [qn.QNRequest(n, g=t(g)), other,
                                   qn.QNRequest(n, J=DeviceCSR(pat, t(val)), v=DVec.from_host(v))]
    x, terms = requests(x0, g0, val0, v0)
    out = lagr.resolve(terms, x)
    assert out[0] is lagr.memory.term and out[1:] == [other]     # the term FIRST
    assert lagr.counts() == (0, 0)
    x, terms = requests(x1, g1, val1, v1)
    out = lagr.resolve(terms, x)
    assert out[0] is lagr.memory.term and getattr(out[0], "lowrank_term", False)
    assert lagr.fused_launches == 1 and lagr.fallback_terms == 0
    state, W = lagr.memory.state.clone(), lagr.memory.W.clone()    # what the update left
    # the same point again with other multipliers: s = 0, not an update, not counted; the ring,
    # the Gram and C stay (only the header's "last update stored its pair" word is cleared)
    x, terms = requests(x1, g1, val1, v0)
    lagr.resolve(terms, x)
    assert lagr.counts() == (1, 0)
    assert torch.equal(lagr.memory.W, W)
    assert torch.equal(lagr.memory.state[:6], state[:6])
    assert torch.equal(lagr.memory.state[8:], state[8:])
    # ... against ipx_lowrank_update called directly with y from the host twin
    y = cases.host_twin(_hip.load(), shape, *cases.transpose(indptr, indices, shape),
                        val_new=val1, val_old=val0, v=v1, base_new=g1, base_old=g0, y0=None,
                        accumulate=False)
    s = (DVec.from_host(x1) - DVec.from_host(x0))
    direct = qn._Memory(strategy, n)
    _hip.call("ipx_lowrank_update", strategy.kind, n, strategy.memory, strategy.init_value,
              strategy.threshold, _p(direct.W), _p(s.t), _p(DVec.from_host(y).t),
              _p(direct.state), _p(direct.part), stream_ptr())
    assert direct.counts() == (1, 0)
    assert torch.equal(state, direct.state)
    assert torch.equal(W, direct.W)
    # the product on s against a float64 numpy compact form
    s_h = s.to_host()
    twin = CompactTwin(strategy.kind, strategy.memory)
    twin.update(s_h, y)
    assert twin.updates == 1
    Bs = lagr.memory.term.dot(DVec.from_host(s_h)).to_host()
    assert _rel(Bs, twin.dot(s_h)) < 1e-12
    if cls is ipsolver.LSR1:
        assert _rel(Bs, y) < 1e-12            # the secant equation of the stored pair


def test_fallback_for_a_dense_jacobian_and_a_changed_pattern():
    from ipsolver import quasi_newton as qn
    n, m = 40, 6
    rng = np.random.default_rng(9)
    lagr = qn.LagrangianQN(ipsolver.LSR1(3), n, host_callbacks=True)
    A0, A1 = rng.standard_normal((m, n)), rng.standard_normal((m, n))
    S0 = sps.random(m, n, 0.3, random_state=1, format="csr")
    S1 = sps.random(m, n, 0.3, random_state=2, format="csr")          # another structure
    x0, x1, v = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(m)
    lagr.resolve([qn.QNRequest(n, J=A0, v=v), qn.QNRequest(n, J=S0, v=v)], x0)
    lagr.resolve([qn.QNRequest(n, J=A1, v=v), qn.QNRequest(n, J=S1, v=v)], x1)
    assert lagr.fallback_terms == 2 and lagr.fused_launches == 0
    y = (A1 - A0).T @ v + (S1 - S0).T @ v
    assert lagr.counts() == (1, 0)
    Bs = lagr.memory.term.dot(lagr._point(x1 - x0)).to_host()
    assert _rel(Bs, y) < 1e-12


# ---- whole solves ---------------------------------------------------------------------------
class _Counted:
    def __init__(self, f):
        self.f, self.calls = f, 0

    def __call__(self, *a):
        self.calls += 1
        return self.f(*a)


def _counted_function(f):
    """a plain function (numpy mode deep-copies the constraints: a function is copied by
    reference, so its counter is the one the test reads)"""
    def g(*a):
        g.calls += 1
        return f(*a)
    g.calls = 0
    return g


def _with_strategy(ns, cons, strategy, counters=None):
    """the problem's constraints with ``strategy`` on every nonlinear one"""
    single = not isinstance(cons, (tuple, list))
    out = []
    for c in ([cons] if single else cons):
        if isinstance(c, ns.NonlinearConstraint):
            jac = _counted_function(c._jac)
            if counters is not None:
                counters.append(jac)
            c = ns.NonlinearConstraint(c._fun, c.kind, jac, strategy, c.enforce_feasibility)
        out.append(c)
    return out[0] if single else tuple(out)


HOST = [problems.Maratos(), problems.HyperbolicIneq()]
DEVICE = [problems.DeviceMaratos(), problems.DeviceHyperbolicIneq()]


def _device_exact_hess(host):
    import torch
    diag = float(host.hess(host.x0)[0, 0])
    return lambda x: torch.full_like(x, diag)


@pytest.mark.parametrize("prob", HOST, ids=[p.name for p in HOST])
def test_no_extra_callbacks_host_mode(prob):
    jacs = []
    grad = _Counted(prob.grad)
    res, _ = run(prob.fun, prob.x0, grad, ipsolver.LSR1(10),
                 _with_strategy(ipsolver, prob.constraints(ipsolver), ipsolver.LSR1(10), jacs))
    print(prob.name, "njev", res.njev, "jac calls", jacs[0].calls, "ngev", res.ngev,
          "grad calls", grad.calls)
    assert len(jacs) == 1 and jacs[0].calls == res.njev
    assert grad.calls == res.ngev
    assert res.hess_updates > 0


@pytest.mark.parametrize("prob", DEVICE, ids=[type(p).__name__ for p in DEVICE])
def test_no_extra_callbacks_device_mode(prob):
    host = type(prob).__mro__[1]()
    # the calls the solver makes by itself in this mode: the same problem with exact Hessians
    exact_grad, exact_jacs = _Counted(prob.grad), []
    cons = prob.constraints(ipsolver)
    nl = cons if isinstance(cons, ipsolver.NonlinearConstraint) else cons[0]
    counted = ipsolver.NonlinearConstraint(nl._fun, nl.kind, _Counted(nl._jac), nl._hess)
    exact_jacs.append(counted._jac)
    exact_cons = counted if isinstance(cons, ipsolver.NonlinearConstraint) \
        else (counted,) + tuple(cons[1:])
    exact, _ = run(prob.fun, prob.device_x0(), exact_grad, _device_exact_hess(host), exact_cons)
    jacs = []
    grad = _Counted(prob.grad)
    res, _ = run(prob.fun, prob.device_x0(), grad, ipsolver.LSR1(10),
                 _with_strategy(ipsolver, prob.constraints(ipsolver), ipsolver.LSR1(10), jacs))
    print(type(prob).__name__, "njev", res.njev, "jac calls", jacs[0].calls, "ngev", res.ngev,
          "grad calls", grad.calls, "| exact: njev", exact.njev, "jac calls",
          exact_jacs[0].calls, "ngev", exact.ngev, "grad calls", exact_grad.calls)
    assert res.hess_updates > 0
    assert jacs[0].calls == res.njev
    # no gradient calls beyond ngev but the solver's own (where a barrier subproblem ends: as
    # many as the exact solve shows for its levels; tests/test_gpu_quasi_newton.py)
    if res.method == "tr_interior_point":
        assert 0 <= grad.calls - res.ngev <= exact_grad.calls - exact.ngev
    else:
        assert grad.calls == res.ngev


def test_loop_form_with_an_exact_csr_objective(monkeypatch):
    """CenteredBandedNLP(2000, 200), device callbacks, LSR1(5) on the constraint, the objective's
    Hessian exact as CSR: the CG loop applies one csr term plus the low-rank term itself"""
    import torch
    from ipsolver import backend_hip, cg_fused, projector
    from ipsolver.synthetic import CenteredBandedNLP, DeviceCallbacks
    dc = DeviceCallbacks(CenteredBandedNLP(2000, 200))
    jac = _Counted(dc.constr_jac)
    seen = []
    plain = backend_hip.hessian_operator

    def spy(terms, n_vars, slack_block):
        H = plain(terms, n_vars, slack_block)
        seen.append(H)
        return H
    monkeypatch.setattr(backend_hip, "hessian_operator", spy)

    def solve():
        con = ipsolver.NonlinearConstraint(dc.constr_fun, ("equals", 0), jac, ipsolver.LSR1(5))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return ipsolver.minimize_constrained(dc.fun, dc.x0, dc.grad, dc.hess, con, max_iter=12)
    monkeypatch.delenv("IPX_DEBUG_FORMS", raising=False)
    ops, calls = cg_fused.STATS["operator_calls"], cg_fused.STATS["calls"]
    res = solve()
    assert cg_fused.STATS["calls"] > calls                        # the device loop ran
    assert cg_fused.STATS["operator_calls"] == ops                # ... with no host products
    assert jac.calls == res.njev
    assert res.hess_updates > 0
    assert len(seen) >= 2
    for H in seen:
        assert H.csr is not None and H.lowrank is not None and getattr(H.lowrank, "lowrank_term")
        assert H.others == () and H.diag is None
        Hc, Hd, LR = cg_fused._loop_parts(H)
        assert Hc is not None and LR is H.lowrank
    A = dc.constr_jac(dc.x0)
    Z, _, _ = projector.projections(A)
    L = cg_fused._Loop(seen[-1], Z.projector, None, None)
    assert L.args.H_operator == 0 and L.args.LR_W and L.args.LR_state
    # the default form against the operator form (tests/test_gpu_quasi_newton_loop.py's demand)
    monkeypatch.setenv("IPX_DEBUG_FORMS", "no-lowrank-loop")
    res_op = solve()
    monkeypatch.delenv("IPX_DEBUG_FORMS")
    assert cg_fused.STATS["operator_calls"] > ops                 # the operator form
    x, x_op = res.x.cpu().numpy(), res_op.x.cpu().numpy()
    print("banded: niter", res.niter, "cg", res.cg_niter, "updates", res.hess_updates,
          "skipped", res.hess_skipped)
    assert (res.niter, res.cg_niter, res.status) == (res_op.niter, res_op.cg_niter, res_op.status)
    assert np.max(np.abs(x - x_op)) <= 1e-12 * max(1.0, np.max(np.abs(x_op)))


_exact_cache = {}


def _exact(host):
    if host.name not in _exact_cache:
        _exact_cache[host.name] = run(host.fun, host.x0, host.grad, host.hess,
                                      host.constraints(ipsolver))[0]
    return _exact_cache[host.name]


def _check(res, exact, label):
    x = res.x.cpu().numpy() if hasattr(res.x, "cpu") else res.x
    print(label, "status", res.status, "niter", res.niter, "cg_niter", res.cg_niter, "updates",
          res.hess_updates, "skipped", res.hess_skipped, "| exact niter", exact.niter,
          "cg_niter", exact.cg_niter)
    assert res.niter <= 1000                            # max_iter (the default)
    assert res.status == 1, (res.status, res.niter)
    assert np.max(np.abs(x - exact.x)) <= 1e-5
    assert res.hess_updates > 0
    return x


@pytest.mark.parametrize("objective", ["exact", "lsr1"])
@pytest.mark.parametrize("prob", HOST, ids=[p.name for p in HOST])
def test_end_to_end_host_callbacks(prob, objective):
    strategy = ipsolver.LSR1(10)
    hess = prob.hess if objective == "exact" else ipsolver.LSR1(10)
    res, _ = run(prob.fun, prob.x0, prob.grad, hess,
                 _with_strategy(ipsolver, prob.constraints(ipsolver), strategy))
    _check(res, _exact(prob), "host %s %s:" % (prob.name, objective))
    assert res.constr_violation <= 1e-8


@pytest.mark.parametrize("objective", ["exact", "lsr1"])
@pytest.mark.parametrize("prob", DEVICE, ids=[type(p).__name__ for p in DEVICE])
def test_end_to_end_device_callbacks(prob, objective, monkeypatch):
    import torch
    host = type(prob).__mro__[1]()
    strategy = ipsolver.LSR1(10)
    hess = _device_exact_hess(host) if objective == "exact" else ipsolver.LSR1(10)

    def solve():
        return run(prob.fun, prob.device_x0(), prob.grad, hess,
                   _with_strategy(ipsolver, prob.constraints(ipsolver), strategy))[0]
    monkeypatch.delenv("IPX_DEBUG_FORMS", raising=False)
    res = solve()
    assert torch.is_tensor(res.x) and res.x.is_cuda
    x = _check(res, _exact(host), "device %s %s:" % (host.name, objective))
    assert res.constr_violation <= 1e-8
    # the default form against the operator form: the agreement the loop test demands
    monkeypatch.setenv("IPX_DEBUG_FORMS", "no-lowrank-loop")
    res_op = solve()
    monkeypatch.delenv("IPX_DEBUG_FORMS")
    x_op = res_op.x.cpu().numpy()
    assert (res.niter, res.cg_niter, res.status) == (res_op.niter, res_op.cg_niter, res_op.status)
    assert np.max(np.abs(x - x_op)) <= 1e-12 * max(1.0, np.max(np.abs(x_op)))
