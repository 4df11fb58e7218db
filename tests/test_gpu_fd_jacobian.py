"""Finite-difference constraint Jacobians on the GPU: the three kernels of csrc/fdjac.hip, the
matrix modes of ``approx_derivative`` and ``minimize_constrained`` with ``jac='2-point'`` /
``'3-point'``, against what the reference's ``_numdiff`` produced on the same inputs
(tests/golden/fd_jac.npz, e2e_fd_jac.json; tests/golden/make_golden_fd_jac.py, tests/fd_cases.py).

Kernels and matrices are held to the reference's bits: the steps, the perturbed points and the
quotients are elementwise, the test functions are built from ``+ - *`` and CSR row sums, which
the device computes as numpy / scipy do.  End-to-end runs are held to the
policy of tests/test_gpu_e2e.py (``compare``) with ``amplify = 10`` (measured: 2.47)."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sps

import ipsolver
import fd_cases
from banded_setup import load_synthetic
from conftest import GOLDEN, load_npz
from test_host_logic import run, compare

pytestmark = pytest.mark.gpu
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


def dev(a, dtype=np.float64):
    import torch
    from ipsolver.device import ctx
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(ctx().device)


def test_steps_kernel_bit_for_bit(gold):
    from ipsolver.fd_jacobian import SparseFDPlan
    x0 = fd_cases.step_x0()
    n = len(x0)
    plan = SparseFDPlan(sps.identity(n, format="csr"), np.zeros(n, dtype=int), n, n)
    for name, (lb, ub) in fd_cases.step_bounds(x0).items():
        forms = [(dev(lb), dev(ub))] + ([None] if name == "none" else [])
        if name == "lower":
            forms.append((dev(lb), np.inf))
        if name == "upper":
            forms.append((-np.inf, dev(ub)))
        for method in METHODS:
            for bounds in forms:
                h, flags = plan.steps(dev(x0), method, bounds)
                tag = "steps_%s_%s" % (name, TAG[method])
                assert same_bits(h.cpu().numpy(), gold[tag + "_h"]), tag
                assert np.array_equal(flags.cpu().numpy().astype(bool), gold[tag + "_os"]), tag
    h, _ = plan.steps(dev(x0), '2-point', None, fd_cases.step_rel(x0))
    assert same_bits(h.cpu().numpy(), gold["steps_rel_h"])


@pytest.mark.parametrize("name,budget", [("tri", None), ("rand", None), ("rand", 30 * 8 * 3),
                                         ("banded", None), ("banded", 200 * 8 * 2 * 4)])
def test_perturb_and_assemble_kernels_bit_for_bit(name, budget, gold, structs):
    """Every perturbed point, dx and the assembled values; with a small budget the assemble runs
    in chunks of groups (one launch per chunk, each writing only its own entries); 'rand' has an
    empty row and an empty column."""
    import torch
    from ipsolver import _hip
    from ipsolver.fd_jacobian import SparseFDPlan
    st = structs[name]
    m, n = st["S"].shape
    groups = gold[name + "_groups0"]
    plan = SparseFDPlan(st["S"], groups, n, m) if budget is None else \
        SparseFDPlan(st["S"], groups, n, m, budget_bytes=budget)
    x0 = dev(st["x0"])
    for bounded in (False, True):
        bounds = tuple(dev(b) for b in fd_cases.case_bounds(st["x0"])) if bounded else None
        for method in METHODS:
            tag = "%s_%s_%s" % (name, TAG[method], "b" if bounded else "u")
            h, flags = plan.steps(x0, method, bounds)
            assert same_bits(h.cpu().numpy(), gold[tag + "_h"]), tag
            dx = torch.full((n,), float("nan"), dtype=torch.float64, device=x0.device)
            for g in range(plan.n_groups):
                x1, x2 = plan.perturb(x0, h, flags, g, method, dx)
                if tag + "_X1" in gold:
                    assert np.array_equal(x1.cpu().numpy(), gold[tag + "_X1"][g]), (tag, g)
                    if x2 is not None:
                        assert np.array_equal(x2.cpu().numpy(), gold[tag + "_X2"][g]), (tag, g)
            assert same_bits(dx.cpu().numpy(), gold[tag + "_dx"]), tag
            # the assemble fed the golden function values, in chunks of the plan's size
            chunk = plan.chunk_groups(method)
            if budget is not None:
                assert chunk < plan.n_groups
            val = torch.full((plan.nnz,), float("nan"), dtype=torch.float64, device=x0.device)
            launches = _hip.load().ipx_launch_count()
            for g_lo in range(0, plan.n_groups, chunk):
                g_hi = min(plan.n_groups, g_lo + chunk)
                F1 = dev(gold[tag + "_F1"][g_lo:g_hi])
                F2 = dev(gold[tag + "_F2"][g_lo:g_hi]) if method == '3-point' else None
                plan.assemble(method, g_lo, g_hi, dev(gold[tag + "_f0"]), F1, F2,
                              dev(gold[tag + "_dx"]), dev(gold[tag + "_os"], np.uint8), val)
            assert _hip.load().ipx_launch_count() - launches == -(-plan.n_groups // chunk)
            assert np.array_equal(plan.pattern.indices_h, gold[tag + "_J_indices"])
            assert np.array_equal(plan.pattern.indptr_h, gold[tag + "_J_indptr"])
            assert same_bits(val.cpu().numpy(), gold[tag + "_J_data"]), tag


def report(tag, got, want, F, dx_min):
    """Prints the largest difference in units of ulp(max|f|) / |dx| before anything is asserted."""
    d = np.max(np.abs(got - want)) if got.size else 0.0
    unit = np.spacing(np.max(np.abs(F))) / dx_min
    print("fd-jacobian %-28s max|diff| %.3e = %.3f x ulp(max|f|)/min|dx|" % (tag, d, d / unit))


@pytest.mark.parametrize("name", ["tri", "banded", "rand"])
def test_approx_derivative_device_and_numpy_modes(name, gold, structs):
    """Device mode (CUDA x0, ``fun`` of separate + - * torch operations and DeviceCSR products)
    and numpy mode against the reference's Jacobian: equal bits."""
    import torch
    from ipsolver._numdiff import approx_derivative
    from ipsolver.device import DeviceCSR, DVec
    st = structs[name]
    groups = gold[name + "_groups0"]
    A = DeviceCSR.from_scipy(st["A"])
    assert A.pattern.nnz == st["A"].nnz
    W = DeviceCSR(A.pattern, dev(st["W"].data))
    b = dev(st["b"])
    half_kappa = 0.5 * fd_cases.KAPPA

    def fun_dev(x):
        return A.dot(DVec(x)).t + half_kappa * W.dot(DVec(x * x)).t - b
    x0 = dev(st["x0"])
    f0_dev = fun_dev(x0).cpu().numpy()
    print("fd-jacobian %s: device f0 equals numpy's: %s" % (name, same_bits(f0_dev, st["fun"](st["x0"]))))
    for bounded in (False, True):
        lb, ub = fd_cases.case_bounds(st["x0"]) if bounded else (-np.inf, np.inf)
        for method in METHODS:
            tag = "%s_%s_%s" % (name, TAG[method], "b" if bounded else "u")
            want = gold[tag + "_J_data"]
            dx_min = np.min(np.abs(gold[tag + "_dx"]))
            J = approx_derivative(st["fun"], st["x0"], method, bounds=(lb, ub),
                                  sparsity=(st["S"], groups))
            assert sps.isspmatrix_csr(J) and J.shape == st["S"].shape
            report(tag + " numpy", J.data, want, gold[tag + "_F1"], dx_min)
            assert np.array_equal(J.indices, gold[tag + "_J_indices"])
            assert np.array_equal(J.indptr, gold[tag + "_J_indptr"])
            assert same_bits(J.data, want), tag
            if method == 'cs':
                continue        # (DeviceCSR products are real: 'cs' runs through numpy mode above)
            bd = (dev(lb), dev(ub)) if bounded else (lb, ub)
            Jd = approx_derivative(fun_dev, x0, method, bounds=bd, sparsity=(st["S"], groups))
            assert isinstance(Jd, DeviceCSR) and Jd.val.is_cuda
            got = Jd.val.cpu().numpy()
            report(tag + " device", got, want, gold[tag + "_F1"], dx_min)
            assert np.array_equal(Jd.pattern.indices_h, gold[tag + "_J_indices"])
            assert same_bits(got, want), tag
    # groups computed from a structure alone; f0 given
    J = approx_derivative(st["fun"], st["x0"], '2-point', f0=st["fun"](st["x0"]), sparsity=st["S"])
    assert same_bits(J.data, gold[name + "_2p_u_J_data"])
    with pytest.raises(ValueError, match="`x0` violates bound constraints."):
        approx_derivative(fun_dev, x0, '2-point', bounds=(dev(st["x0"] + 1.0), np.inf),
                          sparsity=(st["S"], groups))


def test_dense_mode_against_the_reference(gold):
    import torch
    from ipsolver._numdiff import approx_derivative
    from ipsolver.dense import DeviceDense
    for name, case in fd_cases.dense_cases().items():
        want = gold[name + "_J"]
        J = approx_derivative(case["fun"], case["x0"], case["method"], bounds=case["bounds"])
        assert isinstance(J, np.ndarray) and J.shape == want.shape, name
        assert (J.ndim == 1) == (case["m"] == 1)
        assert same_bits(J, want), name
        if case["method"] == 'cs':
            continue
        t = {k: dev(v, np.int64 if v.dtype.kind == "i" else np.float64)
             for k, v in case["tables"].items()}

        def fun_dev(x, t=t):
            return t["a"] * x[t["p"]] * x[t["q"]] + t["c"] * x[t["r"]] - t["d"]
        bounds = tuple(dev(b) for b in case["bounds"]) if np.ndim(case["bounds"][0]) else case["bounds"]
        Jd = approx_derivative(fun_dev, dev(case["x0"]), case["method"], bounds=bounds)
        assert isinstance(Jd, DeviceDense) and Jd.shape == (case["m"], case["n"])
        assert same_bits(Jd.to_host().reshape(want.shape), want), name


def test_check_derivative_is_zero_on_an_exact_jacobian():
    """``f = 2 x``: doubling is exact, so the central quotient is exactly 2."""
    from ipsolver._numdiff import check_derivative
    from ipsolver.device import DeviceCSR
    n = 9
    x0 = np.linspace(-2.0, 2.0, n)
    assert check_derivative(lambda x: 2 * x, lambda x: 2 * sps.identity(n, format="csr"), x0) == 0.0
    assert check_derivative(lambda x: 2 * x, lambda x: 2 * np.eye(n), x0) == 0.0
    assert check_derivative(lambda x: 2 * x, lambda x: 3 * np.eye(n), x0) == 0.5
    J = DeviceCSR.from_scipy(2 * sps.identity(n, format="csr"))
    assert check_derivative(lambda x: 2 * x, lambda x: J, dev(x0)) == 0.0


# ---- end to end -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e_gold():
    with open(os.path.join(GOLDEN, "e2e_fd_jac.json")) as f:
        return json.load(f)


# ``compare``'s amplify: started at 1; the MI355X runs need 2.47 ('2-point': SQP 2.47, barrier
# 1.96) and 1.15 ('3-point': 1.12 / 1.15) times the golden's own one-ulp movement, numpy and
# device callbacks alike -- the next power of ten above the measured ratio
AMPLIFY = 10.0


def banded_problem(gold):
    syn = load_synthetic()
    prob = syn.CenteredBandedNLP(2000, 200, eps=1e-3)
    S = sps.csr_matrix((np.ones(prob.A0.nnz), prob.A0.indices, prob.A0.indptr), shape=prob.A0.shape)
    return prob, S, gold["banded_groups0"]


@pytest.fixture
def evaluations(monkeypatch):
    """Counts the Jacobian evaluations of the solves run under it (``SparseFDPlan.evaluate``)."""
    from ipsolver import fd_jacobian
    seen = []
    real = fd_jacobian.SparseFDPlan.evaluate

    def counting(self, *a, **k):
        seen.append(1)
        return real(self, *a, **k)
    monkeypatch.setattr(fd_jacobian.SparseFDPlan, "evaluate", counting)
    return seen


def check_solve(res, rows, rec, fd, G, evals, method):
    """``jac_fd_nfev``: G (2 G) calls per Jacobian evaluation plus one for f0 at every evaluation
    but the first, where the constraint's own value at x0 is used.  The SQP method evaluates the
    Jacobian ``njev`` times; the barrier method evaluates it again where a new barrier
    subproblem starts at a point its memo no longer holds, which ``njev`` -- the reference's
    count -- leaves out (the same calls a callable ``jac`` gets)."""
    assert res.status == 1
    per = 2 * G if fd == '3-point' else G
    assert res.jac_fd_nfev == evals * per + (evals - 1)
    if method == "equality_constrained_sqp":
        assert evals == res.njev
    else:
        assert evals >= res.njev
    for key in ("status", "niter", "cg_niter", "njev"):
        assert int(res[key]) == rec[key], key
    del res["jac_fd_nfev"]                    # (the reference's result has no such field)
    if hasattr(res.x, "cpu"):
        res.x = res.x.cpu().numpy()
    compare(res, rows, rec, amplify=AMPLIFY)


@pytest.mark.parametrize("fd", ["2-point", "3-point"])
@pytest.mark.parametrize("method", ["equality_constrained_sqp", "tr_interior_point"])
def test_solve_with_numpy_callbacks(method, fd, gold, e2e_gold, evaluations):
    prob, S, groups = banded_problem(gold)
    con = ipsolver.NonlinearConstraint(prob.constr_fun, ("equals", 0), fd, prob.constr_hess,
                                       finite_diff_jac_sparsity=(S, groups))
    res, rows = run(prob.fun, prob.x0, prob.grad, prob.hess, con, method=method)
    rec = e2e_gold["banded_eq_n2000_%s_jac%s" % (method, TAG[fd])]
    assert rec["n_groups"] == 17
    check_solve(res, rows, rec, fd, 17, len(evaluations), method)


@pytest.mark.parametrize("fd", ["2-point", "3-point"])
@pytest.mark.parametrize("method", ["equality_constrained_sqp", "tr_interior_point"])
def test_solve_with_device_callbacks(method, fd, gold, e2e_gold, monkeypatch, evaluations):
    import torch
    from ipsolver import projector, sqp_chain
    from ipsolver.synthetic import DeviceCallbacks
    prob, S, groups = banded_problem(gold)
    dc = DeviceCallbacks(prob)
    made, jac_calls = [], []
    real = projector.BandedNormalSolver.__init__

    def counting(self, *a, **k):
        made.append(1)
        return real(self, *a, **k)
    monkeypatch.setattr(projector.BandedNormalSolver, "__init__", counting)

    def twin_jac(x):
        jac_calls.append(1)
        return dc.constr_jac(x)

    def solve(jac, **kw):
        con = ipsolver.NonlinearConstraint(dc.constr_fun, ("equals", 0), jac, dc.constr_hess, **kw)
        fronts, solvers = sqp_chain.STATS["fronts"], len(made)
        res, rows = run(dc.fun, dc.x0, dc.grad, dc.hess, con, method=method)
        return res, rows, sqp_chain.STATS["fronts"] - fronts, len(made) - solvers
    twin, _, twin_fronts, twin_solvers = solve(twin_jac)
    assert "jac_fd_nfev" not in twin and twin_fronts > 0 and twin_solvers > 0
    res, rows, fronts, solvers = solve(fd, finite_diff_jac_sparsity=(S, groups))
    assert torch.is_tensor(res.x) and res.x.is_cuda
    # the chain stages and the banded solver, exactly as with the callable jac of that pattern
    assert (fronts, solvers) == (twin_fronts, twin_solvers)
    assert res.niter == twin.niter and res.cg_niter == twin.cg_niter
    assert len(evaluations) == len(jac_calls)
    check_solve(res, rows, e2e_gold["banded_eq_n2000_%s_jac%s" % (method, TAG[fd])], fd, 17,
                len(evaluations), method)


def test_refusals_in_device_mode(gold):
    from ipsolver.synthetic import DeviceCallbacks
    prob, S, groups = banded_problem(gold)
    dc = DeviceCallbacks(prob)
    con = ipsolver.NonlinearConstraint(dc.constr_fun, ("equals", 0), '2-point', dc.constr_hess)
    with pytest.raises(ValueError, match="finite_diff_jac_sparsity"):
        ipsolver.minimize_constrained(dc.fun, dc.x0, dc.grad, dc.hess, con)
    con = ipsolver.NonlinearConstraint(dc.constr_fun, ("equals", 0), '2-point', dc.constr_hess,
                                       finite_diff_jac_sparsity=(S, groups))
    with pytest.raises(NotImplementedError, match="row-sharded backend"):
        ipsolver.minimize_constrained(dc.fun, dc.x0, dc.grad, dc.hess, con,
                                      options={"shard": True})
    with pytest.raises(ValueError, match="complex steps do not nest"):
        ipsolver.NonlinearConstraint(dc.constr_fun, ("equals", 0), 'cs', '2-point',
                                     finite_diff_jac_sparsity=(S, groups))
    # a grouping that puts two columns of one row together
    with pytest.raises(ValueError, match="must not share a row"):
        bad = ipsolver.NonlinearConstraint(dc.constr_fun, ("equals", 0), '2-point',
                                           dc.constr_hess,
                                           finite_diff_jac_sparsity=(S, np.zeros(2000, dtype=int)))
        ipsolver.minimize_constrained(dc.fun, dc.x0, dc.grad, dc.hess, bad)


def test_fd_hessian_composes_with_fd_jacobian(gold):
    """``hess`` by differences of ``J(x)'v`` over a finite-difference ``J`` (device callbacks):
    the solve converges to the analytic run's point (to the 1e-6 that
    tests/test_gpu_e2e.py::test_device_callbacks_finite_difference_hessians holds two
    finite-difference runs to: both stop at gtol = 1e-8)."""
    from ipsolver.synthetic import DeviceCallbacks
    syn = load_synthetic()
    prob = syn.CenteredBandedNLP(600, 60, eps=1e-3)
    dc = DeviceCallbacks(prob)
    S = sps.csr_matrix((np.ones(prob.A0.nnz), prob.A0.indices, prob.A0.indptr), shape=prob.A0.shape)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = ipsolver.minimize_constrained(dc.fun, dc.x0, dc.grad, dc.hess,
                                             dc.constraints(ipsolver), method="tr_interior_point")
        got = ipsolver.minimize_constrained(
            dc.fun, dc.x0, dc.grad, dc.hess,
            ipsolver.NonlinearConstraint(dc.constr_fun, ("equals", 0), '3-point', '3-point',
                                         finite_diff_jac_sparsity=S),
            method="tr_interior_point")
    assert got.status == want.status == 1
    assert got.optimality < 1e-8 and got.constr_violation < 1e-8
    xw = want.x.cpu().numpy()
    assert np.max(np.abs(got.x.cpu().numpy() - xw)) <= 1e-6 * np.max(np.abs(xw))
