"""``sparse_rank_deficient = "skip-pivots"`` end to end (tests/test_gpu_sparse_deficient.py has the
solver and the operators):

  * the flow QP of tests/test_gpu_nested_dissection.py at N = 12 on the PURE incidence matrix
    (rank m - 1, a consistent right-hand side), with numpy callbacks and with device callbacks,
    against the reference's own run on the same input (tests/golden/sparse_rank_deficient_e2e.json,
    the rule of tests/test_gpu_rank_deficient_e2e.py::test_redundant_rows_against_the_reference);
  * past the host exit's cap: grid(80, 0.125) with two duplicated rows and a three-term
    combination appended (m n = 1.2e8 > 2^25): a LinAlgError without the option, solved with it,
    judged against the same problem without the three rows on the existing full-rank path;
  * a nonlinear constraint whose sparse Jacobian has a duplicated row at every point: every
    refactorization stays on the device.
Iteration counts are compared nowhere."""
import json
import os
import warnings

import numpy as np
import pytest
import scipy.sparse as sps

import ipsolver
import sparse_deficient_cases as cases
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
OPTION = {"sparse_rank_deficient": "skip-pivots"}
DEVICE_EXIT = "Using a pivot-skipping sparse Cholesky factorization on the device"
GTOL = 1e-8


def solve(A, c, b, mode="numpy", **options):
    """min 1/2 ||x||^2 + c'x  subject to  A x = b -> (result, warnings)"""
    n = A.shape[1]
    if mode == "numpy":
        H = sps.identity(n, format="csr")
        fun, grad, hess = (lambda x: 0.5 * x.dot(x) + c.dot(x)), (lambda x: x + c), (lambda x: H)
        x0, At = np.zeros(n), A
    else:
        import torch
        import ipsolver.device as dv
        dev = torch.device("cuda", torch.cuda.current_device())
        ct = torch.from_numpy(c).to(dev)
        ones = torch.ones(n, dtype=torch.float64, device=dev)
        fun = lambda x: float(0.5 * x.dot(x) + ct.dot(x))            # noqa: E731
        grad = lambda x: x + ct                                       # noqa: E731
        hess = lambda x: ones                                         # noqa: E731  (diagonal)
        x0, At = torch.zeros(n, dtype=torch.float64, device=dev), dv.DeviceCSR.from_scipy(A)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = ipsolver.minimize_constrained(fun, x0, grad, hess,
                                            ipsolver.LinearConstraint(At, ("equals", b)),
                                            gtol=GTOL, options=dict(options))
    return res, [str(w.message) for w in caught]


def host_x(res):
    return res.x if isinstance(res.x, np.ndarray) else res.x.cpu().numpy()


def no_svd(messages):
    return not [t for t in messages if "Using SVD" in t or "dense SVD" in t]


@pytest.mark.parametrize("mode", ["numpy", "device"])
def test_pure_incidence_matrix_against_the_reference(mode):
    """The yardstick is the reference's own result on the same problem measured against the KKT
    point of the independent rows: its distance to it, its objective with its one-ulp movement,
    its constraint violation."""
    with open(os.path.join(GOLDEN, "sparse_rank_deficient_e2e.json")) as f:
        gold = json.load(f)["sparse"]
    A, c, b, ind = cases.e2e_small()
    xs = cases.kkt_point(A[ind], c, b[ind])
    res, messages = solve(A, c, b, mode, **OPTION)
    assert [t for t in messages if DEVICE_EXIT in t], messages
    assert no_svd(messages), messages
    assert res.normal_solver == "PivotSkippingNestedSolver"
    x = host_x(res)
    dist = np.max(np.abs(x - xs)) / np.max(np.abs(xs))
    floor = 8 * EPS * np.max(abs(A).dot(np.abs(x)) + np.abs(b))
    fun, violation = float(res.fun), float(res.constr_violation)
    print("pure G, N = 12, %s: status %d niter %d, distance %.2e (reference %.2e), |fun - ref| "
          "%.2e (one ulp %.2e), violation %.2e (reference %.2e, floor %.2e)"
          % (mode, res.status, res.niter, dist, gold["distance"],
             abs(fun - gold["fun"]) / abs(gold["fun"]), gold["fun_one_ulp"],
             violation, gold["constr_violation"], floor))
    assert int(res.status) in (1, 2)
    assert dist <= 10 * gold["distance"]
    assert abs(fun - gold["fun"]) <= 10 * gold["fun_one_ulp"] * abs(gold["fun"])
    assert violation <= max(100 * gold["constr_violation"], floor)


def test_past_the_cap_of_the_host_exit():
    """m n = 1.2e8 elements: without the option the singular Jacobian ends the solve; with it the
    run is held to what the existing full-rank path does on the same problem without the three
    dependent rows (``sparse_direct="nested-dissection"``): the distance of x to the host KKT
    point of the independent rows may be 10 times that run's, the violation
    max(100 times that run's, its rounding floor)."""
    A, c, b, ind = cases.e2e_large()
    m, n = A.shape
    assert m * n > 1 << 25 and m == len(ind) + 3
    with pytest.raises(np.linalg.LinAlgError, match="too large for the dense SVD fallback"):
        solve(A, c, b)
    xs = cases.kkt_point(A[ind], c, b[ind])
    ref, _ = solve(A[ind], c, b[ind], sparse_direct="nested-dissection")
    assert ref.normal_solver == "NestedDissectionNormalSolver" and int(ref.status) in (1, 2)
    res, messages = solve(A, c, b, **OPTION)
    assert [t for t in messages if DEVICE_EXIT in t] and no_svd(messages), messages
    assert res.normal_solver == "PivotSkippingNestedSolver"
    dist = lambda r: np.max(np.abs(host_x(r) - xs)) / np.max(np.abs(xs))      # noqa: E731
    floor = 8 * EPS * np.max(abs(A).dot(np.abs(host_x(res))) + np.abs(b))
    print("grid(80) + 3 dependent rows: status %d niter %d, distance %.2e (full-rank run %.2e), "
          "violation %.2e (full-rank run %.2e, floor %.2e)"
          % (res.status, res.niter, dist(res), dist(ref), float(res.constr_violation),
             float(ref.constr_violation), floor))
    assert int(res.status) in (1, 2)
    assert dist(res) <= 10 * dist(ref)
    assert float(res.constr_violation) <= max(100 * float(ref.constr_violation), floor)


def test_nonlinear_constraint_with_a_duplicated_row_stays_on_the_device():
    """c(x) = A0 x + kappa/2 W (x*x) - b with W = A0*A0 on the flow rows of the 12 x 12 grid, row
    1 a copy of row 2: the Jacobian ``A0 + kappa W diag(x)`` has the duplicated row at every
    point, so every refactorization of the run meets a rank-deficient matrix and, under the
    option, stays on the device.  The constraints are consistent (``x_feas`` satisfies both
    copies), so the run must end feasible to gtol."""
    A0 = sps.csr_matrix(cases.duplicated(12, ((1, 2),)) / cases.SCALE)
    m, n = A0.shape
    W = A0.multiply(A0).tocsr()
    rng = np.random.default_rng(5)
    kappa, x_feas, q = 0.1, rng.uniform(-1, 1, n), rng.standard_normal(n)
    b = A0.dot(x_feas) + 0.5 * kappa * W.dot(x_feas ** 2)
    x0 = x_feas + 0.1 * rng.standard_normal(n)
    H = sps.identity(n, format="csr")
    con = ipsolver.NonlinearConstraint(
        lambda x: A0.dot(x) + 0.5 * kappa * W.dot(x * x) - b, ("equals", 0),
        lambda x: sps.csr_matrix((A0.data + kappa * W.data * x[A0.indices], A0.indices,
                                  A0.indptr), shape=A0.shape),
        lambda x, v: sps.diags(kappa * W.T.dot(v), format="csr"))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = ipsolver.minimize_constrained(
            lambda x: 0.5 * (x - x_feas).dot(x - x_feas) - 1e-3 * q.dot(x - x_feas), x0,
            lambda x: (x - x_feas) - 1e-3 * q, lambda x: H, con, gtol=GTOL, options=dict(OPTION))
    messages = [str(w.message) for w in caught]
    on_device = [t for t in messages if DEVICE_EXIT in t]
    print("duplicated sparse row: status %d niter %d, %d factorizations on the device, "
          "violation %.2e" % (res.status, res.niter, len(on_device), float(res.constr_violation)))
    assert len(on_device) >= 2, messages
    assert no_svd(messages), messages
    assert res.normal_solver == "PivotSkippingNestedSolver"
    assert int(res.status) in (1, 2)
    assert float(res.constr_violation) <= GTOL
