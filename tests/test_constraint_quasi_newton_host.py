"""Quasi-Newton Hessians on nonlinear constraints without a GPU: the library's host twin of
``ipx_csr_tdiff_dot`` (the pair's ``y``) against a numpy restatement, bit for bit; construction
of ``NonlinearConstraint(hess=<strategy>)``, the equality of strategies and the refusals that
are raised before anything runs on the device."""
import numpy as np
import pytest

import ipsolver
from ipsolver import _hip

import constraint_qn_cases as cases


@pytest.mark.parametrize("with_base", [False, True], ids=["nobase", "base"])
@pytest.mark.parametrize("accumulate", [False, True], ids=["set", "accumulate"])
@pytest.mark.parametrize("name,make", cases.PATTERNS, ids=[n for n, _ in cases.PATTERNS])
def test_host_twin_is_the_numpy_restatement(name, make, accumulate, with_base):
    lib = _hip.load()
    indptr, indices, shape = make()
    t_indptr, t_indices, perm = cases.transpose(indptr, indices, shape)
    if name == "arrow":
        assert t_indptr[1] - t_indptr[0] > _hip.SPMV_TILE_NNZ
    if name == "empty":
        assert np.any(np.diff(t_indptr) == 0) and np.any(np.diff(indptr) == 0)
    op = cases.operands(shape, len(indices), seed=len(indices))
    if not with_base:
        op["base_new"] = op["base_old"] = None
    want = cases.restatement(t_indptr, t_indices, perm, accumulate=accumulate, **op)
    got = cases.host_twin(lib, shape, t_indptr, t_indices, perm, accumulate=accumulate, **op)
    assert np.array_equal(got, want)
    # and it is the product it is meant to be
    import scipy.sparse as sps
    dJ = sps.csr_matrix((op["val_new"] - op["val_old"], indices, indptr), shape=shape)
    ref = dJ.T.dot(op["v"])
    if with_base:
        ref = ref + (op["base_new"] - op["base_old"])
    if accumulate:
        ref = ref + op["y0"]
    assert np.allclose(got, ref, rtol=1e-12, atol=1e-12)


def test_host_twin_refuses_bad_indices():
    lib = _hip.load()
    indptr, indices, shape = cases.tridiagonal()
    t_indptr, t_indices, perm = cases.transpose(indptr, indices, shape)
    op = cases.operands(shape, len(indices), seed=1)
    bad = t_indices.copy()
    bad[3] = shape[0]
    with pytest.raises(AssertionError):
        cases.host_twin(lib, shape, t_indptr, bad, perm, accumulate=False, **op)
    op["base_old"] = None                   # one base vector without the other
    with pytest.raises(AssertionError):
        cases.host_twin(lib, shape, t_indptr, t_indices, perm, accumulate=False, **op)


def test_strategy_equality():
    L, S = ipsolver.LBFGS, ipsolver.LSR1
    assert S() == S(10) == S(10, 'auto', 1e-8)
    assert hash(S()) == hash(S(10))
    assert S(5) != S(6)
    assert S(init_scale=2.0) != S()
    assert S(init_scale=2.0) == S(init_scale=2)
    assert S(min_denominator=1e-6) != S()
    assert L(min_curvature=1e-8) == L()
    assert L() != S()                       # the same fields, another class
    assert S() != "LSR1" and not (S() == None)      # noqa: E711
    assert len({S(), S(10), L(), S(3)}) == 3


def _problem():
    fun = lambda x: float(x @ x)
    grad = lambda x: 2 * x
    cfun = lambda x: np.array([x[0] * x[1] - 1.0])
    cjac = lambda x: np.array([[x[1], x[0], 0.0]])
    return fun, np.ones(3), grad, cfun, cjac


@pytest.mark.parametrize("strategy", [ipsolver.LBFGS(), ipsolver.LSR1(5)])
def test_constraint_constructs_with_a_strategy(strategy):
    _, _, _, cfun, cjac = _problem()
    con = ipsolver.NonlinearConstraint(cfun, ("equals", 0), cjac, hess=strategy)
    assert con._hess is strategy
    # with a finite-difference jac too: it is not refused
    ipsolver.NonlinearConstraint(cfun, ("equals", 0), '2-point', hess=strategy)


def test_unequal_strategies_are_refused_when_the_call_is_made():
    fun, x0, grad, cfun, cjac = _problem()
    calls = []

    def counted(x):
        calls.append(1)
        return fun(x)
    a, b = ipsolver.LSR1(5), ipsolver.LSR1(6)
    con = ipsolver.NonlinearConstraint(cfun, ("equals", 0), cjac, hess=b)
    with pytest.raises(ValueError) as exc:
        ipsolver.minimize_constrained(counted, x0, grad, a, con)
    assert repr(a) in str(exc.value) and repr(b) in str(exc.value)
    # two constraints, the objective exact
    c, d = ipsolver.LBFGS(5), ipsolver.LSR1(5)
    cons = [ipsolver.NonlinearConstraint(cfun, ("equals", 0), cjac, hess=c),
            ipsolver.NonlinearConstraint(cfun, ("less", 3), cjac, hess=d)]
    with pytest.raises(ValueError) as exc:
        ipsolver.minimize_constrained(counted, x0, grad, lambda x: 2 * np.eye(3), cons)
    assert repr(c) in str(exc.value) and repr(d) in str(exc.value)
    assert not calls                        # nothing was evaluated, nothing ran on the device


def test_sharded_backend_is_refused():
    fun, x0, grad, cfun, cjac = _problem()
    con = ipsolver.NonlinearConstraint(cfun, ("equals", 0), cjac, hess=ipsolver.LSR1())
    hess = lambda x: 2 * np.eye(3)
    with pytest.raises(NotImplementedError, match="row-sharded"):
        ipsolver.minimize_constrained(fun, x0, grad, hess, con, options={'shard': True})

    class FakeShardVec:          # what minimize recognises a distributed start vector by
        sh = None
        owns = None
    with pytest.raises(NotImplementedError, match="row-sharded"):
        ipsolver.minimize_constrained(fun, FakeShardVec(), grad, hess, con)


@pytest.mark.parametrize("objective", ["exact", "strategy"])
def test_constant_hessian_is_refused(objective):
    fun, x0, grad, cfun, cjac = _problem()
    con = ipsolver.NonlinearConstraint(cfun, ("equals", 0), cjac, hess=ipsolver.LSR1())
    hess = ipsolver.LSR1() if objective == "strategy" else (lambda x: 2 * np.eye(3))
    with pytest.raises(ValueError, match="constant_hessian"):
        ipsolver.minimize_constrained(fun, x0, grad, hess, con,
                                      options={'constant_hessian': True})
