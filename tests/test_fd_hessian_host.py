"""Sparse finite-difference Hessians without a GPU: the host entry ``ipx_fd_assemble_sym_host``
(the kernel's inline routines on host arrays) against the reference's symmetrised
``approx_derivative`` (tests/golden/fd_hess.npz, made by tests/golden/make_golden_fd_hess.py on
tests/fd_hess_cases.py), chunking, the slot / accumulate form, and the ``SparseFD`` interface with
its refusals."""
import numpy as np
import pytest
import scipy.sparse as sps

import ipsolver
import fd_hess_cases as hc
from banded_setup import load_synthetic
from conftest import load_npz
from ipsolver.fd_hessian import SparseFD, SparseFDHessianPlan, FDTerm

METHODS, TAG = hc.METHODS, hc.TAG
PROBLEMS = ("banded", "tri7", "arrow", "hole")


@pytest.fixture(scope="module")
def gold():
    return load_npz("fd_hess")


@pytest.fixture(scope="module")
def cases():
    return hc.cases(load_synthetic())


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("which", ["grad", "jtv"])
@pytest.mark.parametrize("name", PROBLEMS)
def test_host_entry_equals_the_symmetrised_reference(name, which, gold, cases):
    """Bit for bit, every method; chunked (at least 3 chunks where G allows) equals unchunked;
    the result is exactly symmetric.  The plan is built from the case's own -- possibly
    one-sided -- structure and must arrive at the golden ``S | S'`` and groups."""
    case = cases[name]
    key = "%s_%s" % (name, which)
    plan = SparseFDHessianPlan(case["structures"][which], None, case["n"])
    assert np.array_equal(plan.indptr, gold[key + "_indptr"])
    assert np.array_equal(plan.indices, gold[key + "_indices"])
    assert np.array_equal(plan.groups, gold[key + "_groups"])
    tpos = plan.tpos
    for method in METHODS:
        f0, F1, F2, dx, _, flags = hc.planes(plan, case["funs"][which], case["x0"], method)
        val = plan.assemble_sym_host(method, f0, F1, F2, dx, flags)
        tag = "%s_%s" % (key, TAG[method])
        # the one-sided quotients are the reference's Jacobian
        J = plan.assemble_host(method, f0, F1, F2, dx, flags)
        assert same_bits(J.data, gold[tag + "_J"]), tag
        assert same_bits(val, gold[tag + "_sym"]), tag
        assert same_bits(val, val[tpos]), tag
        if plan.n_groups >= 3:
            chunk = plan.n_groups // 3
            assert -(-plan.n_groups // chunk) >= 3
            got = plan.assemble_sym_host(method, f0, F1, F2, dx, flags,
                                         val=np.full(plan.nnz, np.nan), chunk=chunk)
            assert same_bits(got, val), tag


def test_slot_and_accumulate_add_two_terms_in_order(gold, cases):
    """The objective on the tridiagonal pattern and a constraint on the diagonal, into one array
    on the union pattern: the first term's values, then the second's added."""
    case = cases["banded"]
    pf = SparseFDHessianPlan(case["structures"]["grad"], gold["banded_grad_groups"], case["n"])
    pc = SparseFDHessianPlan(case["structures"]["jtv"], gold["banded_jtv_groups"], case["n"])
    from ipsolver.fd_hessian import LagrangianFDHessian

    class T:
        def __init__(self, plan):
            self.plan = plan
    lag = LagrangianFDHessian()
    lag._plan([T(pf), T(pc)])
    U = sps.csr_matrix((np.ones(len(lag.indices)), lag.indices, lag.indptr), shape=(case["n"],) * 2)
    want_U = hc.sym_pattern(case, "grad") + hc.sym_pattern(case, "jtv")
    assert (U != (want_U != 0)).nnz == 0
    for method in METHODS:
        a = hc.planes(pf, case["funs"]["grad"], case["x0"], method)
        b = hc.planes(pc, case["funs"]["jtv"], case["x0"], method)
        va = pf.assemble_sym_host(method, a[0], a[1], a[2], a[3], a[5])
        vb = pc.assemble_sym_host(method, b[0], b[1], b[2], b[3], b[5])
        val = np.zeros(len(lag.indices))
        pf.assemble_sym_host(method, a[0], a[1], a[2], a[3], a[5], val=val, slot=lag.slots_h[0],
                             accumulate=True)
        pc.assemble_sym_host(method, b[0], b[1], b[2], b[3], b[5], val=val, slot=lag.slots_h[1],
                             accumulate=True)
        want = np.zeros(len(lag.indices))
        want[lag.slots_h[0]] += va
        want[lag.slots_h[1]] += vb
        assert same_bits(val, want), method


def test_accumulate_adds_to_what_is_there(cases):
    case = cases["tri7"]
    plan = SparseFDHessianPlan(case["structures"]["grad"], None, case["n"])
    f0, F1, F2, dx, _, flags = hc.planes(plan, case["funs"]["grad"], case["x0"], '3-point')
    val = plan.assemble_sym_host('3-point', f0, F1, F2, dx, flags)
    base = np.arange(plan.nnz, dtype=float)
    got = plan.assemble_sym_host('3-point', f0, F1, F2, dx, flags, val=base.copy(), accumulate=True)
    assert same_bits(got, base + val)
    # without `accumulate` a chunked run overwrites what was there
    got = plan.assemble_sym_host('3-point', f0, F1, F2, dx, flags, val=base.copy(), chunk=1)
    assert same_bits(got, val)


def test_sparse_fd_arguments():
    S = sps.csr_matrix(np.triu(np.ones((4, 4))))
    s = SparseFD('3-point', sparsity=S, rel_step=1e-6)
    assert not callable(s)
    assert repr(s) == "SparseFD(method='3-point', sparsity=<4 x 4 structure>, groups=None, rel_step=1e-06)"
    assert repr(SparseFD()) == "SparseFD(method='2-point', sparsity=None, groups=None, rel_step=None)"
    assert ipsolver.SparseFD is SparseFD
    for bad in ("4-point", None, 2):
        with pytest.raises(ValueError, match="method must be one of"):
            SparseFD(bad)
    for bad in (np.ones((3, 4)), np.ones(4), "full", sps.csr_matrix(np.ones((2, 3)))):
        with pytest.raises(ValueError, match="sparsity must be"):
            SparseFD(sparsity=bad)
    for bad in ([0.5, 1, 2, 3], [-1, 0, 1, 2], [[0, 1, 2, 3]], [0, 1, 2], "0123"):
        with pytest.raises(ValueError, match="groups"):
            SparseFD(sparsity=S, groups=bad)
    with pytest.raises(ValueError, match="groups need a sparsity structure"):
        SparseFD(groups=[0, 1])
    for bad in (0, -1e-8, np.inf, np.nan, "1e-8", True, [1e-8, 1e-8]):
        with pytest.raises(ValueError, match="rel_step"):
            SparseFD(sparsity=S, rel_step=bad)
    # an asymmetric structure is symmetrised; its grouping is checked like SparseFDPlan's
    plan = FDTerm(SparseFD(sparsity=S), 4, "objective").plan
    assert plan.nnz == 16 and plan.n_groups == 4
    with pytest.raises(ValueError, match="must not share a row"):
        FDTerm(SparseFD(sparsity=S, groups=[0, 0, 1, 2]), 4, "objective")
    with pytest.raises(ValueError, match="4 x 4, the problem has 5 variables"):
        FDTerm(SparseFD(sparsity=S), 5, "objective")
    # no structure: the full pattern, one group per column (numpy callbacks); refused on the device
    plan = FDTerm(SparseFD(), 3, "objective").plan
    assert plan.nnz == 9 and list(plan.groups) == [0, 1, 2]
    with pytest.raises(ValueError, match="needs `sparsity`.*operator form"):
        FDTerm(SparseFD(), 3, "objective", device_mode=True)


def test_refused_combinations():
    """Each names its alternative; all are raised before anything touches a device."""
    import problems
    p = problems.Maratos()
    S = np.ones((2, 2))
    con = p.constraints(ipsolver)
    with pytest.raises(NotImplementedError, match="row-sharded backend; pass an exact Hessian"):
        ipsolver.minimize_constrained(p.fun, p.x0, p.grad, SparseFD(sparsity=S), con,
                                      options={"shard": True})
    nl = ipsolver.NonlinearConstraint(lambda x: x[:1] ** 2, ("equals", 0),
                                      lambda x: np.array([[2 * x[0], 0.0]]), SparseFD(sparsity=S))
    with pytest.raises(NotImplementedError, match="row-sharded backend; pass an exact Hessian"):
        ipsolver.minimize_constrained(p.fun, p.x0, p.grad, p.hess, nl, options={"shard": True})
    with pytest.raises(ValueError, match="constant_hessian.*callable `hess`"):
        ipsolver.minimize_constrained(p.fun, p.x0, p.grad, SparseFD(sparsity=S), con,
                                      options={"constant_hessian": True})
    for jac in ('2-point', '3-point', 'cs'):
        with pytest.raises(ValueError, match="differenced Jacobian; pass a callable `jac`"):
            ipsolver.NonlinearConstraint(lambda x: x, ("equals", 0), jac, SparseFD(sparsity=S))
    with pytest.raises(ValueError, match="differenced Jacobian; pass a callable `jac`"):
        ipsolver.NonlinearConstraint(lambda x: x, ("equals", 0), '2-point',
                                     SparseFD('cs', sparsity=S))
    with pytest.raises(ValueError, match="complex steps do not nest"):      # as before
        ipsolver.NonlinearConstraint(lambda x: x, ("equals", 0), 'cs', '2-point')
