"""Finite-difference constraint Jacobians, the parts that need no GPU: ``group_columns``, the
host entries of csrc/fdjac.hip (the kernels' arithmetic on host arrays) bit for bit against
what the reference's ``_numdiff`` produced (tests/golden/fd_jac.npz, made by
tests/golden/make_golden_fd_jac.py on the inputs of tests/fd_cases.py), the symbolic half of
``SparseFDPlan`` and the argument checks of the public interface."""
import numpy as np
import pytest
import scipy.sparse as sps

import ipsolver
import fd_cases
from banded_setup import load_synthetic
from conftest import load_npz

METHODS, TAG = fd_cases.METHODS, fd_cases.TAG


@pytest.fixture(scope="module")
def gold():
    return load_npz("fd_jac")


@pytest.fixture(scope="module")
def structs():
    return fd_cases.structures(load_synthetic())


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def test_group_columns_equals_the_reference(gold, structs):
    from ipsolver._numdiff import group_columns
    for name, st in structs.items():
        assert np.array_equal(group_columns(st["S"], 0), gold[name + "_groups0"]), name
        assert np.array_equal(group_columns(st["S"]), gold[name + "_groups0"]), name
        assert np.array_equal(group_columns(st["S"], st["order"]), gold[name + "_groups_order"])
        if st["S"].shape[1] <= 64:          # the dense route
            assert np.array_equal(group_columns(st["S"].toarray(), 0), gold[name + "_groups0"])
    assert int(gold["banded_groups0"].max()) + 1 == 17
    with pytest.raises(ValueError, match="`order` has incorrect shape."):
        group_columns(structs["tri"]["S"], np.arange(3))
    with pytest.raises(ValueError, match="`A` must be 2-dimensional."):
        group_columns(np.zeros((2, 2, 2)))


def test_steps_host_bit_for_bit(gold):
    from ipsolver.fd_jacobian import steps_host
    x0 = fd_cases.step_x0()
    checked = 0
    for name, (lb, ub) in fd_cases.step_bounds(x0).items():
        for method in METHODS:
            want_h = gold["steps_%s_%s_h" % (name, TAG[method])]
            want_os = gold["steps_%s_%s_os" % (name, TAG[method])]
            forms = [(lb, ub)]
            if name == "none":
                forms.append((None, None))
            elif name == "lower":
                forms.append((lb, None))
            elif name == "upper":
                forms.append((None, ub))
            for lo, hi in forms:
                h, flags = steps_host(x0, method, None, lo, hi)
                assert same_bits(h, want_h), (name, method)
                assert np.array_equal(flags, want_os), (name, method)
                checked += 1
    assert checked == 3 * 7
    # the cases do what they are there for: flipped, shrunk and one-sided steps all occur
    h2, hn = gold["steps_both_2p_h"], gold["steps_none_2p_h"]
    assert np.any(h2 == -hn) and np.any((np.abs(h2) < np.abs(hn)))
    assert gold["steps_both_3p_os"].any() and not gold["steps_both_3p_os"].all()
    h, _ = steps_host(x0, '2-point', fd_cases.step_rel(x0))
    assert same_bits(h, gold["steps_rel_h"])


@pytest.mark.parametrize("name", ["tri", "banded", "rand"])
def test_perturb_and_assemble_host_bit_for_bit(name, gold, structs):
    from ipsolver.fd_jacobian import SparseFDPlan, perturb_host, steps_host
    st = structs[name]
    m, n = st["S"].shape
    groups = gold[name + "_groups0"]
    plan = SparseFDPlan(st["S"], groups, n, m)
    for bounded in (False, True):
        lb, ub = fd_cases.case_bounds(st["x0"]) if bounded else (None, None)
        for method in METHODS:
            tag = "%s_%s_%s" % (name, TAG[method], "b" if bounded else "u")
            h, flags = steps_host(st["x0"], method, None, lb, ub)
            assert same_bits(h, gold[tag + "_h"]) and np.array_equal(flags, gold[tag + "_os"])
            dx = np.full(n, np.nan)
            for g in range(plan.n_groups):
                x1, x2 = perturb_host(st["x0"], h, flags, groups, g, method, dx)
                if tag + "_X1" in gold:
                    assert np.array_equal(x1, gold[tag + "_X1"][g]), (tag, g)
                    if x2 is not None:
                        assert np.array_equal(x2, gold[tag + "_X2"][g]), (tag, g)
            assert same_bits(dx, gold[tag + "_dx"]), tag
            J = plan.assemble_host(method, gold[tag + "_f0"], gold[tag + "_F1"],
                                   gold.get(tag + "_F2"), gold[tag + "_dx"], gold[tag + "_os"])
            assert np.array_equal(J.indptr, gold[tag + "_J_indptr"]), tag
            assert np.array_equal(J.indices, gold[tag + "_J_indices"]), tag
            assert same_bits(J.data, gold[tag + "_J_data"]), tag
    if name != "tri":
        assert gold[name + "_3p_b_os"].any()


def test_plan_pattern_zeros_and_invalid_groupings(gold, structs):
    from ipsolver.fd_jacobian import SparseFDPlan
    st = structs["rand"]
    m, n = st["S"].shape
    groups = gold["rand_groups0"]
    # unsorted input, stored zeros in the structure: one sorted pattern, zeros dropped
    S = sps.coo_matrix(st["S"])
    perm = np.random.default_rng(0).permutation(S.nnz)
    messy = sps.coo_matrix((np.r_[S.data[perm], 0.0], (np.r_[S.row[perm], 5], np.r_[S.col[perm], 7])),
                           shape=S.shape)
    plan = SparseFDPlan(messy, groups, n, m)
    assert np.array_equal(plan.indptr, st["S"].indptr) and np.array_equal(plan.indices, st["S"].indices)
    assert plan.indptr[6] == plan.indptr[5] and 7 not in plan.indices     # empty row and column
    a = plan.assemble_host('2-point', gold["rand_2p_u_f0"], gold["rand_2p_u_F1"], None,
                           gold["rand_2p_u_dx"], gold["rand_2p_u_os"])
    b = plan.assemble_host('2-point', gold["rand_2p_u_f0"], gold["rand_2p_u_F1"], None,
                           gold["rand_2p_u_dx"], gold["rand_2p_u_os"])
    assert np.array_equal(a.indices, b.indices) and a.nnz == st["S"].nnz
    # entries of the structure on which the function does not depend stay stored, as zeros
    assert np.count_nonzero(a.data == 0) >= st["S"].nnz // 4 and a.nnz == plan.nnz
    # two columns of one group sharing a row: refused, naming the row and the columns
    bad = groups.copy()
    row = int(np.argmax(np.diff(st["S"].indptr) >= 2))
    c0, c1 = st["S"].indices[st["S"].indptr[row]:st["S"].indptr[row] + 2]
    bad[c1] = bad[c0]
    with pytest.raises(ValueError) as exc:
        SparseFDPlan(st["S"], bad, n, m)
    text = str(exc.value)
    assert "row %d" % row in text and "columns %d and %d" % (c0, c1) in text
    with pytest.raises(ValueError, match="groups"):
        SparseFDPlan(st["S"], groups[:-1], n, m)
    with pytest.raises(ValueError, match="shape"):
        SparseFDPlan(st["S"], groups, n, m + 1)
    with pytest.raises(ValueError, match="2\\*\\*31"):
        from ipsolver.fd_jacobian import dense_plan
        dense_plan(1 << 16, 1 << 15)


def test_plan_keeps_one_pattern_object(monkeypatch, structs, gold):
    """The device pattern is built once and is the same object ever after (made here with a
    stand-in for the device class: the identity rule is host logic)."""
    from ipsolver import device
    from ipsolver.fd_jacobian import SparseFDPlan
    made = []

    class FakePattern:
        def __init__(self, indptr, indices, shape):
            made.append(self)
    monkeypatch.setattr(device, "CSRPattern", FakePattern)
    st = structs["tri"]
    plan = SparseFDPlan(st["S"], gold["tri_groups0"], 12, 12)
    assert plan.pattern is plan.pattern and len(made) == 1


def test_approx_derivative_argument_errors():
    from ipsolver._numdiff import approx_derivative, __all__ as names
    assert names == ['approx_derivative', 'group_columns', 'check_derivative']
    f = lambda x: x * x
    x0 = np.array([1.0, 2.0])
    with pytest.raises(ValueError, match="Unknown method 'foo'. "):
        approx_derivative(f, x0, method="foo")
    with pytest.raises(ValueError, match="`x0` must have at most 1 dimension."):
        approx_derivative(f, np.ones((2, 2)), method="2-point")
    with pytest.raises(ValueError, match="Inconsistent shapes between bounds and `x0`."):
        approx_derivative(f, x0, bounds=(np.zeros(3), np.inf))
    with pytest.raises(ValueError, match="`x0` violates bound constraints."):
        approx_derivative(f, x0, bounds=(1.5, np.inf))
    with pytest.raises(ValueError, match="`f0` passed has more than 1 dimension."):
        approx_derivative(f, x0, f0=np.ones((2, 2)))
    with pytest.raises(RuntimeError, match="`fun` return value has more than 1 dimension."):
        approx_derivative(lambda x: np.ones((2, 2)), x0)
    with pytest.raises(ValueError, match="2\\*\\*31"):
        approx_derivative(lambda x: np.zeros(1 << 15), np.zeros(1 << 16), f0=np.zeros(1 << 15))


def test_operator_mode_is_unchanged():
    from ipsolver._numdiff import approx_derivative
    from ipsolver.fd import FiniteDifferenceOperator
    f = lambda x: np.array([x[0] * x[1], x[1] ** 2])
    x0 = np.array([1.0, 2.0])
    for method in METHODS[:2]:
        op = approx_derivative(f, x0, method, as_linear_operator=True)
        assert isinstance(op, FiniteDifferenceOperator) and op.shape == (2, 2)
        p = np.array([0.3, -0.2])
        assert np.array_equal(op.dot(p), FiniteDifferenceOperator(f, x0, method).dot(p))
    with pytest.raises(ValueError, match="Bounds not supported"):
        approx_derivative(f, x0, bounds=(0, 5), as_linear_operator=True)


def test_nonlinear_constraint_arguments():
    NC = ipsolver.NonlinearConstraint
    f, j, h = (lambda x: x), (lambda x: np.eye(2)), (lambda x, v: None)
    c = NC(f, ("equals", 0), j, h, True)                  # positional calls unchanged
    assert (c._hess, c.enforce_feasibility) == (h, True)
    assert c.finite_diff_jac_sparsity is None and c.finite_diff_rel_step is None
    S = np.eye(2)
    c = NC(f, ("equals", 0), '3-point', h, finite_diff_jac_sparsity=S, finite_diff_rel_step=1e-6)
    assert c._jac == '3-point' and c.finite_diff_jac_sparsity is S
    NC(f, ("equals", 0), '2-point')                       # composes with the default hess
    NC(f, ("equals", 0), 'cs', None)
    with pytest.raises(ValueError, match="complex steps do not nest"):
        NC(f, ("equals", 0), 'cs')                        # (hess defaults to '2-point')
    with pytest.raises(ValueError, match="complex steps do not nest"):
        NC(f, ("equals", 0), 'cs', '3-point')
    with pytest.raises(ValueError, match="`jac` must be callable"):
        NC(f, ("equals", 0), '4-point', h)
    with pytest.raises(ValueError, match="finite-difference `jac`"):
        NC(f, ("equals", 0), j, h, finite_diff_jac_sparsity=S)
    with pytest.raises(ValueError, match="finite-difference `jac`"):
        NC(f, ("equals", 0), j, h, finite_diff_rel_step=1e-6)


def test_sharded_backends_refuse_a_string_jac(monkeypatch):
    f = lambda x: x[:1]
    con = ipsolver.NonlinearConstraint(f, ("equals", 0), '2-point', None,
                                       finite_diff_jac_sparsity=np.ones((1, 2)))
    args = (lambda x: 0.0, np.zeros(2), lambda x: x, lambda x: np.eye(2), con)
    with pytest.raises(NotImplementedError, match="row-sharded backend"):
        ipsolver.minimize_constrained(*args, options={"shard": True})
    monkeypatch.setenv("IPX_SHARD", "1")
    with pytest.raises(NotImplementedError, match="jac='2-point'"):
        ipsolver.minimize_constrained(*args)
    monkeypatch.delenv("IPX_SHARD")

    class FakeShardVec:
        sh, owns = object(), object()
    with pytest.raises(NotImplementedError, match="row-sharded backend"):
        ipsolver.minimize_constrained(args[0], FakeShardVec(), *args[2:])
