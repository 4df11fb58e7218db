"""``qp.projected_gltr`` on the device against the exact constrained minimiser, the numpy model
and ``qp.projected_cg``, and ``minimize_constrained(..., options={'subproblem': 'gltr'})`` end to
end with host and device callbacks."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import gltr_cases
import gltr_model
import ipsolver

pytestmark = pytest.mark.gpu

KINDS = ("dense", "csr")
PARAMS = [(c, s, k) for c in sorted(gltr_cases.CASES) for s in gltr_cases.SEEDS for k in KINDS]


@functools.lru_cache(maxsize=None)
def reference(case, seed):
    """The exact constrained minimiser (ii), computed once per problem."""
    H, c, A, b, radius = gltr_cases.problem(case, seed)
    xs, lam, kind = gltr_model.exact_constrained(H, c, A, b, radius)
    return xs, gltr_model.model_value(H, c, xs)


def operators(H, A, kind):
    from ipsolver import device as dv, projector
    from ipsolver.dense import DeviceDense
    if kind == "dense":
        Hd, Ad = DeviceDense.from_host(H), DeviceDense.from_host(A)
    else:
        Hd, Ad = dv.DeviceCSR.from_scipy(sp.csr_matrix(H)), dv.DeviceCSR.from_scipy(sp.csr_matrix(A))
    Z, _, Y = projector.projections(Ad)
    return Hd, Z, Y


def gamma0(H, c, A, b):
    _, g, _ = gltr_model._start(H, c, A, b)
    return np.linalg.norm(g)


@pytest.mark.parametrize("case,seed,kind", PARAMS)
def test_tight_tolerance_reaches_the_exact_minimiser(case, seed, kind):
    from ipsolver import qp
    H, c, A, b, radius = gltr_cases.problem(case, seed)
    xs, qs = reference(case, seed)
    Hd, Z, Y = operators(H, A, kind)
    tol = 1e-24 * gamma0(H, c, A, b) ** 2
    xd, info = qp.projected_gltr(Hd, c, Z, Y, b, radius, tol=tol, max_vectors=256)
    x = xd.to_host()
    q = gltr_model.model_value(H, c, x)
    print(case, seed, kind, info, np.linalg.norm(x - xs) / np.linalg.norm(xs), abs(q - qs) / abs(qs))
    assert info["stop_cond"] == 4
    assert np.linalg.norm(x - xs) <= 1e-10 * np.linalg.norm(xs)
    assert abs(q - qs) <= 1e-12 * abs(qs)
    assert np.linalg.norm(A @ x + (0 if b is None else b)) <= 1e-10
    assert np.linalg.norm(x) <= radius * (1 + 1e-12)
    if case in gltr_cases.ON_BOUNDARY:
        assert abs(np.linalg.norm(x) - radius) <= 1e-10 * radius
        assert info["hits_boundary"] and info["multiplier"] > 0
    x0 = np.zeros(len(c)) if b is None else -A.T @ np.linalg.solve(A @ A.T, b)
    assert abs(info["predicted"] - (q - gltr_model.model_value(H, c, x0))) <= 1e-10


@pytest.mark.parametrize("case,seed,kind", PARAMS)
def test_default_tolerance_against_projected_cg(case, seed, kind):
    from ipsolver import qp
    H, c, A, b, radius = gltr_cases.problem(case, seed)
    Hd, Z, Y = operators(H, A, kind)
    xg, ig = qp.projected_gltr(Hd, c, Z, Y, b, radius)
    xc, ic = qp.projected_cg(Hd, c, Z, Y, np.zeros(A.shape[0]) if b is None else b, radius)
    xg, xc = xg.to_host(), xc.to_host()
    qg, qc = gltr_model.model_value(H, c, xg), gltr_model.model_value(H, c, xc)
    print(case, seed, kind, ig, ic, "gain %.3g" % ((qc - qg) / abs(qc)))
    assert qg <= qc + 1e-12 * abs(qc)
    if case in gltr_cases.GAINS:
        assert qg <= qc - 0.01 * abs(qc)
    if case == "D":
        assert ig["niter"] == ic["niter"]
        assert np.linalg.norm(xg - xc) <= 1e-12 * np.linalg.norm(xc)
        assert ig["multiplier"] == 0 and not ig["hits_boundary"]


@pytest.mark.parametrize("kind", KINDS)
def test_vector_cap_and_early_exits(kind):
    from ipsolver import qp
    H, c, A, b, radius = gltr_cases.problem("A", 0)
    Hd, Z, Y = operators(H, A, kind)
    xd, info = qp.projected_gltr(Hd, c, Z, Y, b, radius, tol=0.0, max_vectors=3)
    x = xd.to_host()
    xm, im = gltr_model.gltr(H, c, A, b, radius, tol=0.0, max_vectors=3)
    assert info["niter"] == 3 and info["stop_cond"] == 1 and im["niter"] == 3
    assert np.linalg.norm(x - xm) <= 1e-12 * np.linalg.norm(xm)
    assert np.linalg.norm(A @ x) <= 1e-10 and np.linalg.norm(x) <= radius * (1 + 1e-12)
    xc, _ = qp.projected_cg(Hd, c, Z, Y, np.zeros(A.shape[0]), radius)
    qc = gltr_model.model_value(H, c, xc.to_host())
    assert gltr_model.model_value(H, c, x) <= qc + 1e-12 * abs(qc)
    # max_iter caps the same way
    _, info = qp.projected_gltr(Hd, c, Z, Y, b, radius, tol=0.0, max_iter=2)
    assert info["niter"] == 2 and info["stop_cond"] == 1
    # the early exits of projected_cg
    H2, c2, A2, b2, _ = gltr_cases.problem("A'", 0)
    Hd2, Z2, Y2 = operators(H2, A2, kind)
    nx0 = np.linalg.norm(A2.T @ np.linalg.solve(A2 @ A2.T, b2))
    with pytest.raises(ValueError, match="does not have a solution"):
        qp.projected_gltr(Hd2, c2, Z2, Y2, b2, 0.5 * nx0)
    with pytest.raises(ValueError, match="does not have a solution"):
        qp.projected_cg(Hd2, c2, Z2, Y2, b2, 0.5 * nx0)
    # x0 on the sphere (the radius is the norm projected_gltr itself forms: the difference is 0)
    from ipsolver import device as dv
    x0d = Y2.dot(-qp._vec(b2))
    xe, ie = qp.projected_gltr(Hd2, c2, Z2, Y2, b2, dv.norm(x0d))
    assert ie["niter"] == 0 and ie["stop_cond"] == 2 and ie["hits_boundary"]
    assert np.array_equal(xe.to_host(), x0d.to_host())
    xt, it = qp.projected_gltr(Hd, c, Z, Y, b, radius, tol=1e9)
    xct, ict = qp.projected_cg(Hd, c, Z, Y, np.zeros(A.shape[0]), radius, tol=1e9)
    assert it["niter"] == 0 and it["stop_cond"] == 4 and not it["hits_boundary"]
    assert {k: it[k] for k in ict} == ict and not xt.to_host().any()
    # no sphere: projected_cg's own behaviour, negative curvature included
    Hb, cb, Ab, bb, _ = gltr_cases.problem("B", 0)
    Hdb, Zb, Yb = operators(Hb, Ab, kind)
    with pytest.raises(ValueError, match="Negative curvature"):
        qp.projected_gltr(Hdb, cb, Zb, Yb, bb, np.inf)
    Hc, cc, Ac, bc, _ = gltr_cases.problem("C", 0)
    Hdc, Zc, Yc = operators(Hc, Ac, kind)
    xi, ii = qp.projected_gltr(Hdc, cc, Zc, Yc, bc, np.inf)
    xci, ici = qp.projected_cg(Hdc, cc, Zc, Yc, np.zeros(Ac.shape[0]), np.inf)
    assert np.array_equal(xi.to_host(), xci.to_host()) and ii["niter"] == ici["niter"]
    with pytest.raises(ValueError, match="max_vectors"):
        qp.projected_gltr(Hd, c, Z, Y, b, radius, max_vectors=257)


def test_banded_problem_through_the_normal_selection():
    from ipsolver import device as dv, projector, qp
    H, c, A, b, radius = gltr_cases.banded_problem()
    Hh, Ah = H.toarray(), A.toarray()
    xs, lam, _ = gltr_model.exact_constrained(Hh, c, Ah, None, radius)
    qs = gltr_model.model_value(Hh, c, xs)
    Hd, Ad = dv.DeviceCSR.from_scipy(H), dv.DeviceCSR.from_scipy(A)
    Z, _, Y = projector.projections(Ad)
    tol = 1e-24 * gamma0(Hh, c, Ah, None) ** 2
    xd, info = qp.projected_gltr(Hd, c, Z, Y, None, radius, tol=tol, max_vectors=256)
    x = xd.to_host()
    q = gltr_model.model_value(Hh, c, x)
    print(info, np.linalg.norm(x - xs) / np.linalg.norm(xs), abs(q - qs) / abs(qs))
    assert info["stop_cond"] == 4 and info["hits_boundary"] and lam > 0
    assert np.linalg.norm(x - xs) <= 1e-10 * np.linalg.norm(xs)
    assert abs(q - qs) <= 1e-12 * abs(qs)
    assert np.linalg.norm(Ah @ x) <= 1e-10
    assert abs(np.linalg.norm(x) - radius) <= 1e-10 * radius


# ---- end to end ----------------------------------------------------------------------------
class _DeviceTwin:
    """A problem of tests/problems.py behind device callbacks: CUDA tensors in and out, the
    values from the host problem's own expressions."""

    def __init__(self, host):
        self.host = host

    @staticmethod
    def _up(a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()

    def x0(self):
        return self._up(self.host.x0)

    def fun(self, x):
        return float(self.host.fun(x.cpu().numpy()))

    def grad(self, x):
        return self._up(self.host.grad(x.cpu().numpy()))

    def hess(self, x):
        return self._up(self.host.hess(x.cpu().numpy()))

    def constraints(self):
        return ipsolver.LinearConstraint(self._up(self.host.A), ("equals", self.host.rhs))


def _solve(prob, hess, mode, subproblem):
    options = {} if subproblem is None else {"subproblem": subproblem}
    if mode == "host":
        res = ipsolver.minimize_constrained(prob.fun, prob.x0, prob.grad, hess,
                                            prob.constraints(ipsolver), options=options)
        return res, np.asarray(res.x)
    twin = _DeviceTwin(prob)
    res = ipsolver.minimize_constrained(twin.fun, twin.x0(), twin.grad,
                                        twin.hess if hess == "exact" else hess,
                                        twin.constraints(), options=options)
    return res, res.x.cpu().numpy()


@pytest.mark.parametrize("hess", ["exact", "lsr1"])
@pytest.mark.parametrize("mode", ["host", "device"])
def test_end_to_end(mode, hess):
    prob = gltr_cases.e2e_problems()[0]
    H0 = prob.hess(np.asarray(prob.x0))
    assert np.linalg.eigvalsh(H0)[0] < 0            # indefinite at the start
    h = (lambda: prob.hess if mode == "host" else "exact") if hess == "exact" else ipsolver.LSR1
    plain, x_plain = _solve(prob, h(), mode, None)
    gltr, x_gltr = _solve(prob, h(), mode, "gltr")
    print("%s/%s outer iterations: steihaug %d (cg %d), gltr %d (products %d; %d calls, %d on "
          "the boundary)" % (mode, hess, plain.niter, plain.cg_niter, gltr.niter, gltr.cg_niter,
                             gltr.gltr_calls, gltr.gltr_boundary_calls))
    assert plain.status in (1, 2) and gltr.status in (1, 2)
    assert np.max(np.abs(x_plain - x_gltr)) <= 1e-6
    assert gltr.gltr_calls > 0 and gltr.gltr_boundary_calls > 0
    assert "multiplier" in gltr.cg_info and "predicted" in gltr.cg_info
    assert "gltr_calls" not in plain and "multiplier" not in plain.cg_info
