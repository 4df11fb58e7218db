"""The host-side table of the device-mode dense canonical Jacobian (canonical.DenseRowPlan:
where every canonical row of a list of constraints lands in the stacked buffer [J_ineq; J_eq])
against the canonical form itself -- ``_RowMap.dense_jac`` / ``sparse_jac`` per constraint,
stacked by ``_stack_dense`` -- on random dense, sparse and box parts of mixed kinds.  No GPU."""
import numpy as np
import pytest
import scipy.sparse as sps

from ipsolver.canonical import DenseRowPlan, _RowMap, _stack_dense
from ipsolver.constraints import check_kind


def random_kind(rng, m):
    """One of every specification form, bounds drawn per row (equalities, one-sided, two-sided
    and infinite rows mixed when the form allows it)."""
    form = rng.integers(0, 4)
    if form == 0:
        return ("equals", rng.standard_normal(m))
    if form == 1:
        return ("greater", rng.standard_normal(m))
    if form == 2:
        return ("less", rng.standard_normal(m))
    lb = rng.standard_normal(m)
    ub = lb + np.abs(rng.standard_normal(m))
    pick = rng.integers(0, 4, m)
    ub[pick == 0] = lb[pick == 0]            # equality rows (lb == ub), anywhere
    lb[pick == 1] = -np.inf
    ub[pick == 2] = np.inf
    return ("interval", lb, ub)


def random_part(rng, n):
    what = rng.integers(0, 3)
    if what == 2:                            # a box: sparse identity
        return sps.eye(n, format="csr"), random_kind(rng, n)
    m = int(rng.integers(1, 9))
    if what == 0:
        J = rng.standard_normal((m, n))
    else:
        J = sps.random(m, n, density=0.3, format="csr", random_state=rng.integers(1 << 30))
    return J, random_kind(rng, m)


@pytest.mark.parametrize("seed", range(12))
def test_plan_equals_the_canonical_dense_stacking(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 12))
    parts = [random_part(rng, n) for _ in range(int(rng.integers(1, 5)))]
    maps, pairs = [], []
    for J, kind in parts:
        rows = _RowMap(check_kind(kind, J.shape[0]), n)
        maps.append((rows.eq, rows.ineq, rows.sign))
        pairs.append(rows.sparse_jac(J) if sps.issparse(J) else rows.dense_jac(J))
    want_ineq, want_eq = _stack_dense(pairs)
    plan = DenseRowPlan(maps)
    got = plan.apply([J for J, _ in parts], n)
    assert (plan.m_ineq, plan.m_eq) == (want_ineq.shape[0], want_eq.shape[0])
    assert np.array_equal(got[:plan.m_ineq], want_ineq)
    assert np.array_equal(got[plan.m_ineq:], want_eq)
    # every row of the buffer is written exactly once
    dst = np.concatenate([d for _, _, d in plan.parts])
    assert np.array_equal(np.sort(dst), np.arange(plan.m))


def test_plan_of_equalities_in_order_is_the_identity():
    eq = np.arange(5)
    plan = DenseRowPlan([(eq, np.empty(0, int), np.empty(0))])
    src, sign, dst = plan.parts[0]
    assert plan.m_ineq == 0 and plan.m_eq == 5 and sign is None
    assert np.array_equal(src, eq) and np.array_equal(dst, eq)


def test_interval_rows_appear_twice_with_both_signs():
    kind = check_kind(("interval", [-1.0, 0.0, -np.inf], [1.0, 0.0, 2.0]), 3)
    rows = _RowMap(kind, 2)
    plan = DenseRowPlan([(rows.eq, rows.ineq, rows.sign)])
    src, sign, dst = plan.parts[0]
    # lower bounds first (sign -1), then upper bounds (+1), then the equality row
    assert list(src) == [0, 0, 2, 1] and list(sign) == [-1, 1, 1, 1] and list(dst) == [0, 1, 2, 3]
    J = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]])
    got = plan.apply([J], 2)
    assert np.array_equal(got, [[-1, -2], [1, 2], [5, 6], [3, 4]])
