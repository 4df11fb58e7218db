"""Sparse finite-difference Hessians on the GPU: ``ipx_fd_assemble_sym`` against its host entry
and the reference's symmetrised ``approx_derivative`` (tests/golden/fd_hess.npz), the two-term
accumulate, the loop form of a ``hess=SparseFD`` solve and end-to-end runs against the reference
given callable Hessians that return the same symmetrised differences
(tests/golden/e2e_fd_hess.json; tests/golden/make_golden_fd_hess.py, tests/fd_hess_cases.py).

Matrices are held to the reference's bits.  End-to-end runs are held to the policy of
tests/test_gpu_e2e.py (``compare``) with ``AMPLIFY`` (below)."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sps

import ipsolver
import fd_hess_cases as hc
from banded_setup import load_synthetic
from conftest import GOLDEN, load_npz
from test_host_logic import run, compare, unjson, EPS

pytestmark = pytest.mark.gpu
METHODS, TAG = hc.METHODS, hc.TAG


@pytest.fixture(scope="module")
def gold():
    return load_npz("fd_hess")


@pytest.fixture(scope="module")
def cases():
    return hc.cases(load_synthetic())


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def dev(a, dtype=np.float64):
    import torch
    from ipsolver.device import ctx
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(ctx().device)


def device_fun(case, name, which):
    """The case's function as a device callback.  Where the device's arithmetic gives numpy's
    bits -- elementwise ``+ - *`` and CSR row sums of short rows -- it is computed on the device;
    ``banded`` grad (a cube) and ``arrow`` grad (a row sum of 2100 terms, summed in another
    order) are computed by numpy behind the same CUDA-tensor interface: this test is about the
    assemble, not about the callback's rounding."""
    from ipsolver.device import DeviceCSR, DVec
    from ipsolver.fd_jacobian import host_callback
    from ipsolver.device import ctx
    if which == "jtv" and name != "banded":
        atv, wtv = dev(case["atv"]), dev(case["wtv"])
        return lambda x: atv + hc.KAPPA * (x * wtv)
    if which == "grad" and name in ("tri7", "hole"):
        A = DeviceCSR.from_scipy(case["A"])
        assert A.pattern.nnz == case["A"].nnz
        W, b = DeviceCSR(A.pattern, dev(case["W"].data)), dev(case["b"])
        return lambda x: A.dot(DVec(x)).t + (0.5 * hc.KAPPA) * W.dot(DVec(x * x)).t - b
    return host_callback(case["funs"][which], ctx().device)


@pytest.mark.parametrize("which", ["grad", "jtv"])
@pytest.mark.parametrize("name", ["banded", "tri7", "arrow", "hole"])
def test_kernel_against_host_entry_and_golden(name, which, gold, cases):
    """numpy and device callbacks, every method ('cs' with numpy callbacks: DeviceCSR products
    are real), one launch and -- pinned by a small budget -- at least 3 chunks of groups:
    ``max|diff| == 0`` against the host entry and the golden, and exactly symmetric."""
    from ipsolver.device import ctx
    from ipsolver.fd_hessian import SparseFDHessianPlan
    from ipsolver.fd_jacobian import host_callback
    case = cases[name]
    key = "%s_%s" % (name, which)
    n, fun = case["n"], case["funs"][which]
    groups = gold[key + "_groups"]
    G = int(groups.max()) + 1
    plan = SparseFDHessianPlan(case["structures"][which], groups, n)
    assert np.array_equal(plan.pattern.indices_h, gold[key + "_indices"])
    tpos = plan.tpos
    x0 = dev(case["x0"])
    callbacks = {"numpy": host_callback(fun, ctx().device), "device": device_fun(case, name, which)}
    for method in METHODS:
        tag = "%s_%s" % (key, TAG[method])
        want = gold[tag + "_sym"]
        f0, F1, F2, dx, _, flags = hc.planes(plan, fun, case["x0"], method)
        host = plan.assemble_sym_host(method, f0, F1, F2, dx, flags)
        assert same_bits(host, want), tag
        budgets = [None]
        if G >= 3:
            budgets.append(8 * n * (2 if method == '3-point' else 1) * (G // 3))
        for budget in budgets:
            p = plan if budget is None else SparseFDHessianPlan(case["structures"][which], groups,
                                                                n, budget_bytes=budget)
            if budget is not None:
                assert -(-G // p.chunk_groups(method)) >= 3
            for mode, cb in callbacks.items():
                if method == 'cs' and mode == "device":
                    continue
                if budget is not None and name == "arrow" and mode == "numpy":
                    continue        # (2100 round trips once more: the chunks do not depend on it)
                before = p.nfev
                got = p.evaluate(cb, x0, method).val.cpu().numpy()
                d = np.max(np.abs(got - want)) if got.size else 0.0
                print("fd-hessian %-22s %-6s budget %-8s max|diff| %.3e" % (tag, mode, budget, d))
                assert same_bits(got, want), (tag, mode, budget)
                assert same_bits(got, got[tpos]), (tag, mode, budget)
                calls = (2 * G if method == '3-point' else G) + (method != 'cs')
                assert p.nfev - before == calls


@pytest.mark.parametrize("budget", [None, 8 * 2000 * 2])
def test_two_terms_accumulate_into_the_union_pattern(budget, gold, cases):
    """The objective (tridiagonal) plus one constraint (diagonal) in one array on the union of
    their patterns, against the host twin: the first term's values, then the second's added.
    With the small budget the first term runs in chunks through its own scratch array."""
    from ipsolver.fd_hessian import (SparseFD, FDTerm, LagrangianFDHessian, SparseFDHessianPlan)
    case = cases["banded"]
    n, x0 = case["n"], case["x0"]
    specs = [SparseFD('3-point', case["structures"][w], gold["banded_%s_groups" % w])
             for w in ("grad", "jtv")]
    terms = [FDTerm(s, n, "objective") for s in specs]
    if budget is not None:
        for t, w in zip(terms, ("grad", "jtv")):
            t.plan = SparseFDHessianPlan(case["structures"][w], gold["banded_%s_groups" % w], n,
                                         budget_bytes=budget)
        assert terms[0].plan.chunk_groups('3-point') < terms[0].plan.n_groups
    lag = LagrangianFDHessian(host_callbacks=True)
    reqs = [t.request(case["funs"][w], lambda w=w: case["funs"][w](x0))
            for t, w in zip(terms, ("grad", "jtv"))]
    H = lag.evaluate(x0, reqs)
    H2 = lag.evaluate(x0, reqs)
    assert H2.pattern is H.pattern and H2.val is not H.val
    want = np.zeros(H.pattern.nnz)
    for t, w, slot in zip(terms, ("grad", "jtv"), lag.slots_h):
        f0, F1, F2, dx, _, flags = hc.planes(t.plan, case["funs"][w], x0, '3-point')
        want[slot] += t.plan.assemble_sym_host('3-point', f0, F1, F2, dx, flags)
    got = H.val.cpu().numpy()
    assert same_bits(got, want) and same_bits(H2.val.cpu().numpy(), want)
    M = H.to_scipy()
    assert (M != M.T).nnz == 0


# ---- end to end -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e_gold():
    with open(os.path.join(GOLDEN, "e2e_fd_hess.json")) as f:
        return json.load(f)


# ``compare``'s amplify: the ratio a run needs over the golden's own
# one-ulp movement is printed by ``needed_amplify`` below before anything is asserted.  NOT YET
# MEASURED on an MI355X: 10 is the figure of the finite-difference Jacobian runs (measured 2.47,
# test_gpu_fd_jacobian.py), whose quotients these are; the first measurement replaces it by the
# next round figure above the measured ratio
AMPLIFY = 10.0


def needed_amplify(rows, rec, rtol=1e-10):
    """The smallest ``amplify`` with which ``compare`` accepts the float columns of ``rows``."""
    want = np.array([[np.nan if isinstance(v, str) and v == "nan" else v for v in r]
                     for r in unjson(rec["trace"])], dtype=float)
    got = np.array(rows, dtype=float)
    stable = int(rec["one_ulp"]["stable_rows"])
    sens = np.array(unjson(rec["one_ulp"]["rows"]), dtype=float).reshape(stable, 8)
    k = min(stable, len(got))
    need = 0.0
    for col in (2, 3, 4, 5, 6):
        a, b = got[:k, col], want[:k, col]
        ok = np.isfinite(b) & np.isfinite(a)
        if not ok.any():
            continue
        floor = 256 * EPS * np.max(np.abs(want[:, col][np.isfinite(want[:, col])]))
        over = np.abs(a[ok] - b[ok]) - rtol * np.abs(b[ok]) - floor
        s = sens[:k, col][ok]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(over > 0, over / s, 0.0)
        need = max(need, float(np.max(r)))
    return need


def banded(gold, cases):
    case = cases["banded"]
    return (case["prob"], case["structures"]["grad"], gold["banded_grad_groups"],
            case["structures"]["jtv"], gold["banded_jtv_groups"])


@pytest.fixture
def hessians(monkeypatch):
    """What every Hessian operator of the solves run under it was built from."""
    from ipsolver import backend_hip
    seen = []
    real = backend_hip.hessian_operator

    def recording(terms, n_vars, slack_block):
        seen.append(terms.flat_terms())
        return real(terms, n_vars, slack_block)
    monkeypatch.setattr(backend_hip, "hessian_operator", recording)
    return seen


def check_solve(res, rows, rec, fd, hessians, tag):
    """Counters: G_f (2 G_f) gradient calls and G_c (2 G_c) Jacobian calls per Hessian
    evaluation -- the values at the Hessian's point come from the memos --; the reference's
    integers exactly; floats by ``compare``."""
    from ipsolver.device import DeviceCSR
    assert res.status == 1
    evals = len(hessians)
    per = 2 if fd == '3-point' else 1
    assert evals > 0
    assert res.hess_fd_ngev == per * rec["n_groups_f"] * evals
    assert res.hess_fd_njev == per * rec["n_groups_c"] * evals
    # the loop form of an exact CSR Hessian: ONE csr term on one pattern object, nothing else
    assert all(len(t) == 1 and isinstance(t[0], DeviceCSR) for t in hessians)
    assert len({id(t[0].pattern) for t in hessians}) == 1
    for key in ("status", "niter", "cg_niter", "nfev", "njev"):
        assert int(res[key]) == rec[key], key
    del res["hess_fd_ngev"], res["hess_fd_njev"]        # (the reference's result has neither)
    if hasattr(res.x, "cpu"):
        res.x = res.x.cpu().numpy()
    print("fd-hessian e2e %-44s needs amplify %.3f" % (tag, needed_amplify(rows, rec)))
    compare(res, rows, rec, amplify=AMPLIFY)


@pytest.mark.parametrize("fd", ["2-point", "3-point"])
@pytest.mark.parametrize("method", ["equality_constrained_sqp", "tr_interior_point"])
def test_solve_with_numpy_callbacks(method, fd, gold, cases, e2e_gold, hessians):
    prob, Sf, gf, Sc, gc = banded(gold, cases)
    con = ipsolver.NonlinearConstraint(prob.constr_fun, ("equals", 0), prob.constr_jac,
                                       ipsolver.SparseFD(fd, Sc, gc))
    res, rows = run(prob.fun, prob.x0, prob.grad, ipsolver.SparseFD(fd, Sf, gf), con,
                    method=method)
    key = "banded_eq_n2000_%s_hess%s" % (method, TAG[fd])
    check_solve(res, rows, e2e_gold[key], fd, hessians, key + " numpy")


@pytest.mark.parametrize("fd", ["2-point", "3-point"])
@pytest.mark.parametrize("method", ["equality_constrained_sqp", "tr_interior_point"])
def test_solve_with_device_callbacks(method, fd, gold, cases, e2e_gold, hessians):
    """Also the loop form: no host-callback and no ``device_operator`` term (``check_solve``
    sees every operator's terms), and a result on the device."""
    import torch
    from ipsolver.synthetic import DeviceCallbacks
    prob, Sf, gf, Sc, gc = banded(gold, cases)
    dc = DeviceCallbacks(prob)
    con = ipsolver.NonlinearConstraint(dc.constr_fun, ("equals", 0), dc.constr_jac,
                                       ipsolver.SparseFD(fd, Sc, gc))
    res, rows = run(dc.fun, dc.x0, dc.grad, ipsolver.SparseFD(fd, Sf, gf), con, method=method)
    assert torch.is_tensor(res.x) and res.x.is_cuda
    key = "banded_eq_n2000_%s_hess%s" % (method, TAG[fd])
    check_solve(res, rows, e2e_gold[key], fd, hessians, key + " device")


def test_fewer_gradient_calls_than_the_operator_form(gold, cases):
    """``hess='2-point'`` calls the gradient inside every CG iteration; ``SparseFD`` calls it
    G_f times per outer iteration.  Also: a CSRPattern as ``sparsity``, and the refusal of a
    device solve without one."""
    from ipsolver.device import CSRPattern
    from ipsolver.synthetic import DeviceCallbacks
    prob, Sf, gf, Sc, gc = banded(gold, cases)
    dc = DeviceCallbacks(prob)
    calls = []

    def grad(x):
        calls.append(1)
        return dc.grad(x)
    counts = {}
    pat = CSRPattern(Sf.indptr, Sf.indices, Sf.shape)
    for name, hess in (("operator", '2-point'), ("sparse", ipsolver.SparseFD('2-point', pat))):
        del calls[:]
        res, _ = run(dc.fun, dc.x0, grad, hess, dc.constraints(ipsolver),
                     method="equality_constrained_sqp")
        assert res.status == 1
        counts[name] = len(calls)
    print("fd-hessian gradient calls per solve: %r" % (counts,))
    assert counts["sparse"] < counts["operator"]
    assert res.hess_fd_njev == 0 and res.hess_fd_ngev > 0
    with pytest.raises(ValueError, match="needs `sparsity`"):
        ipsolver.minimize_constrained(dc.fun, dc.x0, dc.grad, ipsolver.SparseFD(),
                                      dc.constraints(ipsolver))


def test_sparse_fd_next_to_an_exact_term(gold, cases, hessians):
    """A SparseFD objective next to the exact diagonal constraint Hessian keeps today's handling
    of mixed terms: the differenced CSR first (the operator's ``csr``), the diagonal after it;
    the solve ends at the all-exact run's point."""
    from ipsolver.device import DeviceCSR, DVec
    from ipsolver.synthetic import DeviceCallbacks
    prob, Sf, gf, Sc, gc = banded(gold, cases)
    dc = DeviceCallbacks(prob)
    want, _ = run(dc.fun, dc.x0, dc.grad, dc.hess, dc.constraints(ipsolver),
                  method="equality_constrained_sqp")
    del hessians[:]
    got, _ = run(dc.fun, dc.x0, dc.grad, ipsolver.SparseFD('3-point', Sf, gf),
                 dc.constraints(ipsolver), method="equality_constrained_sqp")
    assert all(isinstance(t[0], DeviceCSR) and isinstance(t[1], DVec) and len(t) == 2
               for t in hessians)
    assert got.status == want.status == 1 and got.niter == want.niter
    xw = want.x.cpu().numpy()
    # '3-point' quotients of a cubic gradient: relative error ~ eps^(2/3) ~ 4e-11 in H, and the
    # solves stop at gtol = 1e-8 -- the bar two finite-difference runs are held to elsewhere
    assert np.max(np.abs(got.x.cpu().numpy() - xw)) <= 1e-6 * np.max(np.abs(xw))
