"""``dense_factorization = "householder-qr"`` end to end (part 5 of tests/test_gpu_dense_qr.py):
BASELINE config 2's recipe at n = 300, m = 60 with a Jacobian of prescribed condition number
(tests/dense_qr_cases.py), and one dense problem with inequality rows in device-callback mode.
Iteration counts are compared nowhere: the reference's own trace on this problem moves from 14
to 23 outer iterations under one unit in the last place of ``c``."""
import json
import os
import warnings

import numpy as np
import pytest

import ipsolver
import dense_qr_cases as cases
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
OPTION = {"dense_factorization": "householder-qr"}


def solve(A, H, c, b, options):
    fun, grad, hess = cases.objective(H, c)
    return ipsolver.minimize_constrained(fun, np.zeros(A.shape[1]), grad, hess,
                                         ipsolver.LinearConstraint(A, ("equals", b)),
                                         method="equality_constrained_sqp", options=options)


def test_well_conditioned_agrees_with_the_default():
    """cond(A) = 1, numpy callbacks: the tolerances of
    test_config2_full_solve_against_reference_trace."""
    A, H, c, b = cases.problem(1.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        default = solve(A, H, c, b, {})
        qr = solve(A, H, c, b, OPTION)
    assert default.normal_solver == "DenseNormalSolver"
    assert qr.normal_solver == "DenseQRProjector"
    assert default.status in (1, 2) and qr.status in (1, 2)
    x_err = np.max(np.abs(qr.x - default.x)) / np.max(np.abs(default.x))
    f_err = abs(qr.fun - default.fun) / abs(default.fun)
    print("cond 1: x %.2e, fun %.2e apart (niter %d / %d)" % (x_err, f_err, default.niter, qr.niter))
    assert x_err <= 1e-7
    assert f_err <= 1e-12


@pytest.mark.parametrize("cond", cases.CONDS)
def test_ill_conditioned_against_the_reference(cond):
    """The yardstick is the reference's own result on the same problem
    (tests/golden/dense_qr_e2e.json) measured against the KKT point: its distance to it, its
    objective with its one-ulp movement, its constraint violation."""
    with open(os.path.join(GOLDEN, "dense_qr_e2e.json")) as f:
        gold = json.load(f)["cond_%.0e" % cond]
    A, H, c, b = cases.problem(cond)
    xs = cases.kkt_point(A, H, c, b)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = solve(A, H, c, b, OPTION)
    messages = [str(w.message) for w in caught]
    assert not [t for t in messages if "Singular" in t or "Ill-conditioned" in t], messages
    assert res.normal_solver == "DenseQRProjector"
    x = np.asarray(res.x)
    dist = np.max(np.abs(x - xs)) / np.max(np.abs(xs))
    floor = 8 * EPS * np.max(np.abs(A).dot(np.abs(x)) + np.abs(b))
    print("cond %.0e: status %d niter %d, distance %.2e (reference %.2e), |fun - ref| %.2e "
          "(one ulp %.2e), violation %.2e (reference %.2e, floor %.2e)"
          % (cond, res.status, res.niter, dist, gold["distance"],
             abs(res.fun - gold["fun"]) / abs(gold["fun"]), gold["fun_one_ulp"],
             res.constr_violation, gold["constr_violation"], floor))
    assert res.status in (1, 2)
    assert dist <= 10 * gold["distance"]
    assert abs(res.fun - gold["fun"]) <= 10 * gold["fun_one_ulp"] * abs(gold["fun"])
    assert res.constr_violation <= max(100 * gold["constr_violation"], floor)


def test_device_callbacks_with_inequality_rows():
    """Device-callback mode, a dense LinearConstraint of mixed kind (the augmented Jacobian
    ``[[J_eq, 0], [J_ineq, diag(s)]]`` of tests/test_gpu_dense_inequality.py, factored as a
    general matrix): option on against the default, status in (1, 2), x to 1e-7.

    Both runs are made with ``xtol = gtol = 1e-10``.  The comparison is of two runs of the barrier
    method that stop on their own optimality measure, and a run that stops at optimality < gtol
    leaves x determined to about gtol x the conditioning of the reduced problem, not better:
    tests/test_gpu_dense_inequality.py records 2.8e-7 between the reference and this package on
    this problem at the default 1e-8.  Measured here at 1e-8: the two runs stop after 56 and 49
    iterations at optimality 9.6e-9 and 7.1e-9, 4.7e-8 and 4.3e-7 from the optimum (a run at
    1e-12) and 4.1e-7 from each other -- the stopping rule's width, above the 1e-7 asked of x.
    At 1e-10 both are 2.4e-9 from the optimum and 1.5e-10 apart, so 1e-7 separates a wrong
    projection from a right one with three orders to spare."""
    from ipsolver.synthetic import CenteredDenseNLP, DenseDeviceCallbacks, mixed_interval_kind
    prob = CenteredDenseNLP(300, 60)
    kind = mixed_interval_kind(60)
    cb = DenseDeviceCallbacks(prob)
    out = {}
    for name, options in (("default", {}), ("qr", OPTION)):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out[name] = ipsolver.minimize_constrained(
                cb.fun, cb.x0, cb.grad, cb.hess, ipsolver.LinearConstraint(cb.A, kind),
                method="tr_interior_point", xtol=1e-10, gtol=1e-10, options=options)
    default, qr = out["default"], out["qr"]
    assert default.normal_solver == "DenseNormalSolver"
    assert qr.normal_solver == "DenseQRProjector"
    assert int(default.status) in (1, 2) and int(qr.status) in (1, 2)
    xd, xq = default.x.cpu().numpy(), qr.x.cpu().numpy()
    x_err = np.max(np.abs(xq - xd)) / np.max(np.abs(xd))
    print("device callbacks: x %.2e apart (niter %d / %d)" % (x_err, default.niter, qr.niter))
    assert x_err <= 1e-7
