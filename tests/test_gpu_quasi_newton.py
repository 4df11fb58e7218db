"""Quasi-Newton Hessians on the GPU: the update and product kernels (csrc/lowrank.hip) against
the numpy twin, and ``minimize_constrained(..., hess=LBFGS() | LSR1())`` end to end in both
callback modes."""
import warnings

import numpy as np
import pytest
from scipy.sparse.linalg import LinearOperator

import ipsolver
import problems
from quasi_newton_twin import CompactTwin
from test_host_logic import run

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b)))


def _pairs(kind, n, count, rng):
    """pairs y = d * s with a pair that is skipped -- negative curvature (L-BFGS), y - Bs
    orthogonal to s (L-SR1) -- and s = 0 among them"""
    d = rng.uniform(0.5, 20.0, n) if kind == 0 else rng.uniform(-5.0, 10.0, n)
    twin = CompactTwin(kind, n)
    out = []
    for k in range(count):
        s = rng.standard_normal(n)
        out.append((s, d * s))
        twin.update(*out[-1])
        if k == 2:
            s = rng.standard_normal(n)
            if kind == 0:
                out.append((s, -s))
            else:
                t = rng.standard_normal(n)
                t -= (t @ s) / (s @ s) * s
                out.append((s, twin.dot(s) + t))
        if k == 5:
            out.append((np.zeros(n), np.zeros(n)))
    return out


def _device_sequence(strategy, pairs, n, probes):
    from ipsolver import _hip, quasi_newton as qn
    from ipsolver.device import DVec, _p, stream_ptr
    mem = qn._Memory(strategy, n)
    out = []
    for s, y in pairs:
        sd, yd = DVec.from_host(s), DVec.from_host(y)
        st = strategy
        _hip.call("ipx_lowrank_update", st.kind, n, st.memory, st.init_value, st.threshold,
                  _p(mem.W), _p(sd.t), _p(yd.t), _p(mem.state), _p(mem.part), stream_ptr())
        out.append([mem.term.dot(DVec.from_host(p)).t.clone() for p in probes])
    return mem, out


@pytest.mark.parametrize("cls,kind", [(ipsolver.LBFGS, 0), (ipsolver.LSR1, 1)])
@pytest.mark.parametrize("memory", [3, 10])
def test_update_and_product_on_device_vectors(cls, kind, memory):
    import torch
    n = 100_000
    rng = np.random.default_rng(memory + 7 * kind)
    pairs = _pairs(kind, n, 2 * memory + 2, rng)            # wraps the ring
    probes = [rng.standard_normal(n), pairs[1][0]]
    twin = CompactTwin(kind, memory)
    strategy = cls(memory)
    mem, seq = _device_sequence(strategy, pairs, n, probes)
    for (s, y), prods in zip(pairs, seq):
        twin.update(s, y)
        for p, bp in zip(probes, prods):
            assert _rel(bp.cpu().numpy(), twin.dot(p)) < 1e-12
    assert mem.counts() == (twin.updates, twin.skipped)
    assert twin.skipped >= 1
    # determinism: a second memory from scratch gives the same bits
    mem2, seq2 = _device_sequence(strategy, pairs, n, probes)
    assert torch.equal(mem.state, mem2.state) and torch.equal(mem.W, mem2.W)
    for a, b in zip(seq, seq2):
        for u, v in zip(a, b):
            assert torch.equal(u, v)


def test_product_in_z_space_with_slack_rows():
    from ipsolver import backend_hip
    from ipsolver.device import DVec
    n, m = 50_000, 7_000
    rng = np.random.default_rng(1)
    pairs = _pairs(0, n, 6, rng)
    probe = rng.standard_normal(n + m)
    twin = CompactTwin(0, 4)
    mem, _ = _device_sequence(ipsolver.LBFGS(4), pairs, n, [])
    for s, y in pairs:
        twin.update(s, y)
    slack = rng.uniform(0.1, 2.0, m)
    H = backend_hip.hessian_operator([mem.term], n, DVec.from_host(slack))
    out = H.dot(DVec.from_host(probe)).to_host()
    assert _rel(out[:n], twin.dot(probe[:n])) < 1e-12
    assert _rel(out[n:], slack * probe[n:]) < 1e-14


def test_accumulating_product():
    from ipsolver.device import DVec
    n = 4097
    rng = np.random.default_rng(2)
    pairs = _pairs(1, n, 5, rng)
    twin = CompactTwin(1, 5)
    mem, _ = _device_sequence(ipsolver.LSR1(5), pairs, n, [])
    for s, y in pairs:
        twin.update(s, y)
    p, base = rng.standard_normal(n), rng.standard_normal(n)
    out = DVec.from_host(base)
    mem.term.dot(DVec.from_host(p), out=out, accumulate=True)
    assert _rel(out.to_host(), base + twin.dot(p)) < 1e-12


class _Counted:
    def __init__(self, f):
        self.f, self.calls = f, 0

    def __call__(self, *a):
        self.calls += 1
        return self.f(*a)


def _cases():
    out = []
    for p in problems.exact_hessian_problems():
        for name, strategy in (("lbfgs", ipsolver.LBFGS()), ("lsr1", ipsolver.LSR1())):
            marks = ()
            if p.name.startswith("elec") and name == "lbfgs":
                # the Coulomb energy has negative curvature along the steps the barrier takes:
                # s'y < 0, every pair after the first few is skipped, B stops changing and the
                # solve runs out of iterations -- the skip rule doing what it says
                marks = pytest.mark.xfail(strict=True, reason="objective curvature negative "
                                          "along the steps: L-BFGS skips every pair")
            out.append(pytest.param(p, strategy, marks=marks,
                                    id="%s%d-%s" % (p.name, len(p.x0), name)))
    return out


@pytest.mark.parametrize("prob,strategy", _cases())
def test_end_to_end_host_callbacks(prob, strategy):
    exact, _ = run(prob.fun, prob.x0, prob.grad, prob.hess, prob.constraints(ipsolver))
    grad = _Counted(prob.grad)
    res, _ = run(prob.fun, prob.x0, grad, strategy, prob.constraints(ipsolver))
    assert res.status in (1, 2), (res.status, res.niter)
    if prob.name.startswith("elec"):
        # electrons on a sphere: the minimiser is unique up to a rotation -- the energy is not
        assert abs(res.fun - exact.fun) <= 1e-7 * abs(exact.fun)
    else:
        assert np.max(np.abs(res.x - exact.x)) <= 1e-5
    assert res.constr_violation <= 1e-8
    assert grad.calls == res.ngev                  # no hidden gradient calls
    assert res.hess_updates + res.hess_skipped >= 1
    assert "hess_updates" not in exact and "hess_skipped" not in exact
    # the same object again: the same bits
    res2, _ = run(prob.fun, prob.x0, prob.grad, strategy, prob.constraints(ipsolver))
    assert np.array_equal(res.x, res2.x) and res.niter == res2.niter


DEVICE = [problems.DeviceMaratos(), problems.DeviceHyperbolicIneq()]


@pytest.mark.parametrize("strategy", [ipsolver.LBFGS(), ipsolver.LSR1()],
                         ids=["lbfgs", "lsr1"])
@pytest.mark.parametrize("prob", DEVICE, ids=[type(p).__name__ for p in DEVICE])
def test_end_to_end_device_callbacks(prob, strategy, monkeypatch):
    import torch
    from ipsolver import quasi_newton as qn
    misses = []
    plain_lookup = qn.DeviceGradientMemo.lookup

    def lookup(self, xt):
        before = self.misses
        g = plain_lookup(self, xt)
        misses.append(self.misses - before)
        return g
    monkeypatch.setattr(qn.DeviceGradientMemo, "lookup", lookup)
    host = type(prob).__mro__[1]()
    exact, _ = run(host.fun, host.x0, host.grad, host.hess, host.constraints(ipsolver))
    # the same problem with its exact (constant, diagonal) Hessian as a device callback: the
    # gradient calls the solver makes by itself in this mode
    diag = float(host.hess(host.x0)[0, 0])
    exact_grad = _Counted(prob.grad)
    exact_dev, _ = run(prob.fun, prob.device_x0(), exact_grad,
                       lambda x: torch.full_like(x, diag), prob.constraints(ipsolver))
    grad = _Counted(prob.grad)
    res, _ = run(prob.fun, prob.device_x0(), grad, strategy, prob.constraints(ipsolver))
    assert torch.is_tensor(res.x) and res.x.is_cuda
    assert res.status in (1, 2)
    assert np.max(np.abs(res.x.cpu().numpy() - exact.x)) <= 1e-5
    assert res.constr_violation <= 1e-8
    # every Hessian request found the gradient the solver had evaluated at its point: the
    # strategy made no gradient call of its own ...
    assert len(misses) >= res.hess_updates and sum(misses) == 0
    # ... so every call beyond ngev is the solver's own: with the exact Hessian it evaluates the
    # gradient again where a barrier subproblem ends (not counted in ngev) -- at most once per
    # barrier level, as many as the exact solve shows for its levels
    if method_is_barrier(res):
        assert 0 <= grad.calls - res.ngev <= exact_grad.calls - exact_dev.ngev, \
            (grad.calls, res.ngev, exact_grad.calls, exact_dev.ngev)
    else:
        assert grad.calls == res.ngev
    assert res.hess_updates + res.hess_skipped >= 1


def method_is_barrier(res):
    return res.method == "tr_interior_point"


def _twin_hessian(kind, memory, grad):
    """test-side ``hess`` callable: the twin's B as a LinearOperator (the operator path)"""
    twin = CompactTwin(kind, memory)
    last = {}

    def hess(x):
        x = np.array(x, dtype=float)
        if "x" in last and np.array_equal(x, last["x"]):
            pass
        else:
            g = np.asarray(grad(x), dtype=float)
            if "x" in last:
                twin.update(x - last["x"], g - last["g"])
            last["x"], last["g"] = x, g
        S, Y, sigma = list(twin.S), list(twin.Y), twin.sigma
        n = len(x)
        return LinearOperator((n, n), matvec=lambda p: twin._apply(S, Y, sigma, np.ravel(p)))
    return hess


@pytest.mark.parametrize("cls,kind", [(ipsolver.LBFGS, 0), (ipsolver.LSR1, 1)])
def test_against_a_twin_operator_through_the_operator_path(cls, kind):
    prob = problems.Rosenbrock(10)

    def solve(hess):
        rows = []

        def cb(state):
            rows.append((np.array(state.x, dtype=float), float(state.optimality),
                         int(state.niter), int(state.cg_niter), int(state.nfev)))
            return False
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = ipsolver.minimize_constrained(prob.fun, prob.x0, prob.grad, hess,
                                                prob.constraints(ipsolver), callback=cb)
        return res, rows
    ref, ref_rows = solve(_twin_hessian(kind, 5, prob.grad))
    res, rows = solve(cls(5))
    assert res.status == ref.status
    assert len(rows) >= 10 and len(ref_rows) >= 10
    for (x, opt, *ints), (x_r, opt_r, *ints_r) in zip(rows[:10], ref_rows[:10]):
        np.testing.assert_allclose(x, x_r, rtol=1e-9, atol=1e-12)             # x
        np.testing.assert_allclose(opt, opt_r, rtol=1e-9, atol=1e-12)         # optimality
        assert ints == ints_r                                                   # niter, cg, nfev


def test_mixed_with_a_finite_difference_constraint_hessian():
    prob = problems.Maratos()
    con = prob.constraints(ipsolver)
    fd_con = ipsolver.NonlinearConstraint(con._fun, con.kind, con._jac, '2-point')
    exact, _ = run(prob.fun, prob.x0, prob.grad, prob.hess, con)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res, _ = run(prob.fun, prob.x0, prob.grad, ipsolver.LBFGS(), fd_con)
    assert res.status in (1, 2)
    assert np.max(np.abs(res.x - exact.x)) <= 1e-5
    assert res.constr_violation <= 1e-8
