"""``rank_deficient = "pivoted-qr"`` end to end (part 5 of tests/test_gpu_rank_deficient.py): the
dense-QR problem (BASELINE config 2's recipe at n = 300, m = 60) scaled by 2^-10 with six
consistent combination rows added and the rows permuted (tests/rank_deficient_cases.py), against
the reference's own result on the same input (tests/golden/rank_deficient_e2e.json), with numpy
callbacks and with device callbacks; and a nonlinear dense constraint whose Jacobian has a
duplicated row at every point.  Iteration counts are compared nowhere
(tests/test_gpu_dense_qr_e2e.py)."""
import json
import os
import warnings

import numpy as np
import pytest

import ipsolver
import dense_qr_cases
import rank_deficient_cases as cases
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
OPTION = {"rank_deficient": "pivoted-qr"}
DEVICE_EXIT = "Using a pivoted QR decomposition on the device"


def solve(A, H, c, b, mode):
    if mode == "numpy":
        fun, grad, hess = dense_qr_cases.objective(H, c)
        x0, At = np.zeros(A.shape[1]), A
    else:
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        At, Ht, ct = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (A, H, c))
        fun = lambda x: float(0.5 * x.dot(Ht @ x) + ct.dot(x))      # noqa: E731
        grad = lambda x: Ht @ x + ct                                  # noqa: E731
        hess = lambda x: Ht                                           # noqa: E731
        x0 = torch.zeros(A.shape[1], dtype=torch.float64, device=dev)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = ipsolver.minimize_constrained(fun, x0, grad, hess,
                                            ipsolver.LinearConstraint(At, ("equals", b)),
                                            method="equality_constrained_sqp",
                                            options=dict(OPTION))
    return res, [str(w.message) for w in caught]


@pytest.mark.parametrize("mode", ["numpy", "device"])
@pytest.mark.parametrize("cond", cases.E2E_CONDS)
def test_redundant_rows_against_the_reference(cond, mode):
    """The yardstick is the reference's own result on the same problem measured against the KKT
    point of the independent rows: its distance to it, its objective with its one-ulp movement,
    its constraint violation (the rule of test_ill_conditioned_against_the_reference)."""
    with open(os.path.join(GOLDEN, "rank_deficient_e2e.json")) as f:
        gold = json.load(f)["cond_%.0e" % cond]
    A, H, c, b, ind = cases.e2e_problem(cond)
    xs = dense_qr_cases.kkt_point(A[ind], H, c, b[ind])
    res, messages = solve(A, H, c, b, mode)
    assert [t for t in messages if DEVICE_EXIT in t], messages
    assert not [t for t in messages if "Using SVD" in t or "dense SVD" in t], messages
    assert res.normal_solver == "DenseCODProjector"
    x = res.x if isinstance(res.x, np.ndarray) else res.x.cpu().numpy()
    dist = np.max(np.abs(x - xs)) / np.max(np.abs(xs))
    floor = 8 * EPS * np.max(np.abs(A).dot(np.abs(x)) + np.abs(b))
    fun, violation = float(res.fun), float(res.constr_violation)
    print("cond %.0e %s: status %d niter %d, distance %.2e (reference %.2e), |fun - ref| %.2e "
          "(one ulp %.2e), violation %.2e (reference %.2e, floor %.2e)"
          % (cond, mode, res.status, res.niter, dist, gold["distance"],
             abs(fun - gold["fun"]) / abs(gold["fun"]), gold["fun_one_ulp"],
             violation, gold["constr_violation"], floor))
    assert int(res.status) in (1, 2)
    assert dist <= 10 * gold["distance"]
    assert abs(fun - gold["fun"]) <= 10 * gold["fun_one_ulp"] * abs(gold["fun"])
    assert violation <= max(100 * gold["constr_violation"], floor)


def test_nonlinear_constraint_with_a_duplicated_row_stays_on_the_device():
    """``CenteredDenseNLP``'s constraint with row 57 a copy of row 5: the Jacobian
    ``A + kappa W diag(x)`` has the duplicated row at every point, so every refactorization of the
    run meets a rank-deficient matrix.  Under the option each of them stays on the device.
    The constraints are consistent (``x_feas`` satisfies both copies), so the run must end
    feasible: the violation is asked to be below gtol = 1e-8, the bound the stopping rule itself
    sets for status 1 (measured: status 1 after 13 iterations, 13 factorizations, 7.1e-15)."""
    from ipsolver.synthetic import CenteredDenseNLP, DenseDeviceCallbacks
    prob = CenteredDenseNLP(300, 60)
    prob.A[57] = prob.A[5]
    prob.W = prob.A * prob.A
    prob.b = prob.A.dot(prob.x_feas) + 0.5 * prob.kappa * prob.W.dot(prob.x_feas ** 2)
    cb = DenseDeviceCallbacks(prob)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = ipsolver.minimize_constrained(cb.fun, cb.x0, cb.grad, cb.hess,
                                            cb.constraints(ipsolver),
                                            method="equality_constrained_sqp",
                                            options=dict(OPTION))
    messages = [str(w.message) for w in caught]
    on_device = [t for t in messages if DEVICE_EXIT in t]
    print("duplicated row: status %d niter %d, %d factorizations on the device, violation %.2e"
          % (res.status, res.niter, len(on_device), float(res.constr_violation)))
    assert len(on_device) >= 2, messages
    assert not [t for t in messages if "Using SVD" in t or "dense SVD" in t], messages
    assert res.normal_solver == "DenseCODProjector"
    assert int(res.status) in (1, 2)
    assert float(res.constr_violation) <= 1e-8
