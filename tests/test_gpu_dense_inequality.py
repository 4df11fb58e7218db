"""Dense constraint Jacobians with inequality rows in device-callback mode (csrc/densejac.hip,
device_mode.DenseStack, dense.AugmentedDense): end to end against the reference's traces, the
constant-Jacobian factorization count, and the kernels bit for bit against numpy."""
import json
import os
import types

import numpy as np
import pytest
import torch

import ipsolver
import problems
from conftest import GOLDEN, unjson
from test_host_logic import run, compare, trace_policy  # noqa: F401

pytestmark = pytest.mark.gpu

F64 = torch.float64


def cuda(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64), dtype=F64, device="cuda")


def dense_ineq_golden():
    with open(os.path.join(GOLDEN, "e2e_dense_ineq.json")) as f:
        return json.load(f)


# ---- the textbook problems with dense device Jacobians -----------------------------------
class DenseHyperbolicIneq(problems.HyperbolicIneq):
    """README example: the nonlinear row's Jacobian a 1 x 2 CUDA tensor, the box next to it."""

    def fun(self, x):
        return float(0.5 * (x[0] - 2) ** 2 + 0.5 * (x[1] - 0.5) ** 2)

    def grad(self, x):
        return torch.stack([x[0] - 2, x[1] - 0.5])

    def hess(self, x):
        return torch.eye(2, dtype=F64, device="cuda")

    def constraints(self, ns, linear=False):
        nl = ns.NonlinearConstraint(
            lambda x: (1 / (x[0] + 1) - x[1]).reshape(1), ("greater", 0.25),
            lambda x: torch.stack([-1 / (x[0] + 1) ** 2, -torch.ones_like(x[0])]).reshape(1, 2),
            lambda x, v: torch.stack([2 * v[0] / (x[0] + 1) ** 3, torch.zeros_like(x[0])]))
        return (nl, ns.BoxConstraint(("greater",)))


class _DeviceRosenbrock:
    def fun(self, x):
        return float(torch.sum(100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (1 - x[:-1]) ** 2))

    def grad(self, x):
        g = torch.zeros_like(x)
        g[:-1] += -400 * x[:-1] * (x[1:] - x[:-1] ** 2) - 2 * (1 - x[:-1])
        g[1:] += 200 * (x[1:] - x[:-1] ** 2)
        return g

    def hess(self, x):
        off = -400 * x[:-1]
        dg = torch.zeros_like(x)
        dg[:-1] = 1200 * x[:-1] ** 2 - 400 * x[1:] + 2
        dg[1:] += 200
        return torch.diag(dg) + torch.diag(off, 1) + torch.diag(off, -1)


def _dense_linear(ns, A, kind, linear):
    """The same rows as a LinearConstraint of a 2-D CUDA tensor or as a NonlinearConstraint
    whose ``jac`` returns one."""
    At = cuda(A)
    if linear:
        return ns.LinearConstraint(At, kind)
    return ns.NonlinearConstraint(lambda x: At @ x, kind, lambda x: At, None)


class DenseIneqRosenbrock(_DeviceRosenbrock, problems.IneqRosenbrock):
    def constraints(self, ns, linear=True):
        return _dense_linear(ns, [[1, 2]], ("less", 1), linear)


class DenseEqIneqRosenbrock(_DeviceRosenbrock, problems.EqIneqRosenbrock):
    def constraints(self, ns, linear=True):
        return (_dense_linear(ns, [[1, 2]], ("less", 1), linear),
                _dense_linear(ns, [[2, 1]], ("equals", 1), linear))


CASES = [(DenseHyperbolicIneq, False), (DenseIneqRosenbrock, True),
         (DenseIneqRosenbrock, False), (DenseEqIneqRosenbrock, True),
         (DenseEqIneqRosenbrock, False)]


@pytest.mark.parametrize("cls,linear", CASES,
                         ids=["%s-%s" % (c.__name__, "linear" if l else "jac") for c, l in CASES])
def test_textbook_problems_with_dense_device_jacobians(cls, linear, e2e_golden):
    p = cls()
    res, rows = run(p.fun, cuda(p.x0), p.grad, p.hess, p.constraints(ipsolver, linear=linear))
    gold = e2e_golden[p.name]
    assert torch.is_tensor(res.x) and res.x.is_cuda and res.s.is_cuda and res.v.is_cuda
    res.x = res.x.cpu().numpy()
    compare(res, rows, gold, **trace_policy(p.name))
    np.testing.assert_array_almost_equal(res.x, p.x_opt, decimal=5)


# ---- the mixed-kind dense NLP against the reference ------------------------------------------
@pytest.mark.parametrize("mode", ["device", "host"])
def test_mixed_kind_dense_nlp_vs_reference(mode):
    from ipsolver.synthetic import CenteredDenseNLP, DenseDeviceCallbacks, mixed_interval_kind
    gold = dense_ineq_golden()["dense_ineq_n300"]
    prob = CenteredDenseNLP(300, 60)
    kind = mixed_interval_kind(60)
    cb = prob if mode == "host" else DenseDeviceCallbacks(prob)
    res, rows = run(cb.fun, cb.x0, cb.grad, cb.hess, cb.constraints(ipsolver, kind),
                    method="tr_interior_point")
    if mode == "device":
        assert all(torch.is_tensor(res[k]) and res[k].is_cuda for k in ("x", "v", "s"))
        res.x, res.v, res.s = (res[k].cpu().numpy() for k in ("x", "v", "s"))
    compare_late_barrier(res, rows, gold)
    for k in ("v", "s"):
        want = np.asarray(unjson(gold[k]))
        err = np.max(np.abs(np.asarray(res[k]) - want)) / np.max(np.abs(want))
        print("%s: max relative difference from the reference %.2e" % (k, err))
        # (the multipliers are least-squares estimates at that x: 3.5e-4 apart in either mode)
        assert err <= 1e-3, k


def compare_late_barrier(res, rows, gold, late=6, counters=True, x_rtol=1e-6):
    """The trace against the reference's, held to what the projections' factorization leaves
    determined.  The golden's one-ulp record perturbs the gradient only; the reference factors
    with a pivoted QR, this package with the Cholesky of A A', and on these dense barrier runs
    that moves the late, small optimality / violation values by up to ~3e-11 absolute and the
    CG count of late steps (row 44 of 46 of dense_ineq_n300: 589 against 578) -- identically in
    host-callback mode, whose arithmetic this feature leaves as it was.  So: the leading rows'
    integer columns exact, their float columns to 1e-8 relative + 1e-9 of the column's largest
    value; then the outcome and the optimum (to 1e-6: both runs stop at gtol = 1e-8 in
    optimality, x differs by 2.8e-7 relative in either callback mode)."""
    want = np.array([[np.nan if v == "nan" else v for v in r] for r in unjson(gold["trace"])],
                    dtype=float)
    got = np.array(rows, dtype=float)
    k = len(want) - late
    assert len(got) >= k
    for col in (0, 1, 7):
        assert np.array_equal(got[:k, col], want[:k, col]), col
    for col in (2, 3, 4, 5, 6):
        a, b = got[:k, col], want[:k, col]
        ok = np.isfinite(b)
        assert np.array_equal(np.isfinite(a), ok)
        scale = np.max(np.abs(want[:, col][np.isfinite(want[:, col])]))
        assert np.all(np.abs(a[ok] - b[ok]) <= 1e-8 * np.abs(b[ok]) + 1e-9 * scale), col
    assert int(res.status) == gold["status"]
    if counters:
        for key in ("niter", "cg_niter", "nfev", "njev"):
            assert int(res[key]) == gold[key], key
    gx = np.asarray(unjson(gold["x"]), dtype=float)
    x = np.asarray(res.x)[::max(1, np.size(res.x) // 50)]
    err = np.max(np.abs(x - gx)) / np.max(np.abs(gx))
    print("x: max relative difference from the reference %.2e" % err)
    assert err <= x_rtol


def test_constant_dense_jacobian_keeps_its_gram(monkeypatch):
    """A dense LinearConstraint with inequality rows: J J' is formed once per solve, every
    assembled augmented Jacobian is factored once (a shift of the kept Gram, Cholesky, inverse),
    nothing is uploaded from the host -- and the trace is the reference's."""
    from ipsolver import _hip
    from ipsolver.dense import DeviceDense
    from ipsolver.synthetic import CenteredDenseNLP, DenseDeviceCallbacks, mixed_interval_kind
    gold = dense_ineq_golden()["dense_lin_ineq_n300"]
    prob = CenteredDenseNLP(300, 60)
    cb = DenseDeviceCallbacks(prob)
    lin = ipsolver.LinearConstraint(cb.A, mixed_interval_kind(60))
    counts = {}
    real_call, real_upload = _hip.call, DeviceDense.from_host

    def counting(name, *args):
        counts[name] = counts.get(name, 0) + 1
        return real_call(name, *args)

    def upload(a):
        counts["from_host"] = counts.get("from_host", 0) + 1
        return real_upload(a)
    monkeypatch.setattr(_hip, "call", counting)
    monkeypatch.setattr(DeviceDense, "from_host", staticmethod(upload))
    res, rows = run(cb.fun, cb.x0, cb.grad, cb.hess, lin, method="tr_interior_point")
    monkeypatch.undo()
    print("constant dense J: %s, njev %d" % (
        {k: counts.get(k, 0) for k in ("ipx_gram_f64_mfma_split", "ipx_gram_shift",
                                       "ipx_chol_factor", "ipx_dense_augment",
                                       "ipx_dense_gather_rows", "from_host")}, res.njev))
    assert counts.get("ipx_gram_f64_mfma_split", 0) == 1
    assert counts.get("ipx_dense_gather_rows", 0) == 1          # the stack, built once
    assert counts.get("from_host", 0) == 0
    n_aug = counts["ipx_dense_augment"]
    assert counts["ipx_chol_factor"] == counts["ipx_chol_inverse"] == n_aug
    assert counts["ipx_gram_shift"] == n_aug
    # one assembled (and factored) augmented Jacobian per Jacobian evaluation -- the initial point
    # and every accepted step -- and one for the barrier subproblem's first slack vector
    assert n_aug <= res.njev + 1
    res.x = res.x.cpu().numpy()
    # (a constant J: the reference's own trace moves by 1.3e-9 in x under one ulp of the
    # gradient, and the CG counts of the second half of the run are not determined beyond the
    # factorization's rounding: 476 against 479 from row 32 on -- the leading rows, the outcome
    # and the optimum are compared)
    compare_late_barrier(res, rows, gold, late=len(gold["trace"]) - 16, counters=False)
    assert res.optimality < 1e-8 and res.constr_violation < 1e-8


# ---- the kernels against numpy, bit for bit ------------------------------------------------
def _call(name, *args):
    from ipsolver import _hip
    from ipsolver.device import stream_ptr
    _hip.call(name, *(list(args) + [stream_ptr()]))


def _p(t):
    return None if t is None else t.data_ptr()


@pytest.mark.parametrize("rows,ncols,src_rows,lds,ldo,col0", [
    (1, 1, 1, 1, 1, 0), (7, 33, 5, 33, 35, 1), (65, 129, 40, 130, 131, 2),
    (300, 1001, 120, 1001, 1004, 3), (17, 2048, 9, 2048, 2050, 2)])
def test_gather_rows_parity(rows, ncols, src_rows, lds, ldo, col0):
    rng = np.random.default_rng(rows * 7 + ncols)
    src = rng.standard_normal((src_rows, lds))
    idx = rng.integers(0, src_rows, rows).astype(np.int32)           # duplicated rows
    sign = rng.choice([-1.0, 1.0], rows)
    out_rows = rows + 3
    dst = rng.permutation(out_rows)[:rows].astype(np.int32)
    fill = rng.standard_normal((out_rows, ldo))
    # (every device operand is held by a name until the launch is done: a temporary's block
    # would go back to the caching allocator and could be handed to the next operand)
    src_d, sign_d = cuda(src), cuda(sign)
    idx_d, dst_d = torch.from_numpy(idx).cuda(), torch.from_numpy(dst).cuda()
    for with_sign in (True, False):
        out = cuda(fill)
        _call("ipx_dense_gather_rows", rows, ncols, _p(src_d), lds, _p(idx_d),
              _p(sign_d) if with_sign else None, _p(dst_d), _p(out), ldo, col0)
        want = fill.copy()
        block = src[idx, :ncols]
        want[dst, col0:col0 + ncols] = block * sign[:, None] if with_sign else block
        assert np.array_equal(out.cpu().numpy(), want)
    # idx / dst omitted: rows in order
    out = cuda(fill[:rows])
    _call("ipx_dense_gather_rows", min(rows, src_rows), ncols, _p(src_d), lds, None, None,
          None, _p(out), ldo, col0)
    want = fill[:rows].copy()
    k = min(rows, src_rows)
    want[:k, col0:col0 + ncols] = src[:k, :ncols]
    assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("rows,ncols,src_rows", [(1, 1, 1), (9, 31, 6), (130, 517, 70)])
def test_csr_rows_to_dense_parity(rows, ncols, src_rows):
    import scipy.sparse as sps
    rng = np.random.default_rng(rows + ncols)
    S = sps.random(src_rows, ncols, density=0.2, format="csr", random_state=rows)
    # a duplicated column entry in row 0 (summed, like toarray does)
    indptr = S.indptr.copy()
    indices = np.concatenate(([0, 0], S.indices))
    data = np.concatenate(([0.25, -1.5], S.data))
    indptr[1:] += 2
    S = sps.csr_matrix((data, indices, indptr), shape=(src_rows, ncols))
    idx = rng.integers(0, src_rows, rows).astype(np.int32)
    idx[0] = 0
    sign = rng.choice([-1.0, 1.0], rows)
    dst = rng.permutation(rows).astype(np.int32)
    ldo = ncols + 3
    out = cuda(rng.standard_normal((rows, ldo)))
    keep = out.cpu().numpy()
    ops = [torch.from_numpy(indptr.astype(np.int32)).cuda(),
           torch.from_numpy(indices.astype(np.int32)).cuda(), cuda(data),
           torch.from_numpy(idx).cuda(), cuda(sign), torch.from_numpy(dst).cuda()]
    _call("ipx_csr_rows_to_dense", rows, ncols, *[_p(o) for o in ops], _p(out), ldo)
    want = keep.copy()
    want[dst, :ncols] = S[idx].toarray() * sign[:, None]
    assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("m_eq,m_in,n", [(0, 1, 1), (0, 5, 7), (3, 2, 5), (37, 45, 129),
                                         (1, 70, 3), (64, 33, 65), (5, 0, 9)])
def test_augment_and_transpose_parity(m_eq, m_in, n):
    from ipsolver import dense
    from ipsolver.device import DVec
    rng = np.random.default_rng(m_eq * 1000 + m_in * 10 + n)
    Je, Ji = rng.standard_normal((m_eq, n)), rng.standard_normal((m_in, n))
    s = rng.uniform(0.1, 2.0, m_in)
    want = np.block([[Je, np.zeros((m_eq, m_in))], [Ji, np.diag(s)]])
    A = dense.augment(cuda(Je).reshape(m_eq, n), cuda(Ji).reshape(m_in, n), DVec(cuda(s)),
                      n, m_eq, m_in)
    assert np.array_equal(A.t.cpu().numpy(), want)
    assert np.array_equal(A.T.t.cpu().numpy(), want.T)
    # the transpose alone (an equality-only stack's SQP matrix)
    D = dense.DeviceDense(cuda(Je).reshape(m_eq, n)) if m_eq else None
    if D is not None:
        dense.transpose_into(D)
        assert np.array_equal(D.T.t.cpu().numpy(), Je.T)


@pytest.mark.parametrize("m,m_eq,incs", [(1, 0, 1), (50, 20, 1), (64, 64, 1), (130, 7, 9)])
def test_gram_shift_parity(m, m_eq, incs):
    from ipsolver import _hip
    M = int(_hip.load().ipx_dense_padded(m))
    rng = np.random.default_rng(m + m_eq)
    G0 = rng.standard_normal((M, M))
    sfull = rng.standard_normal((max(m - m_eq, 1) * incs,))
    s = sfull[::incs][:m - m_eq]
    want = G0.copy()
    i = np.arange(m_eq, m)
    want[i, i] = want[i, i] + s * s
    G = torch.empty((M, M), dtype=F64, device="cuda")
    G0_d, s_d = cuda(G0), cuda(sfull)
    _call("ipx_gram_shift", m, m_eq, _p(G0_d), _p(s_d), incs, _p(G))
    assert np.array_equal(G.cpu().numpy(), want)
    G = cuda(G0)
    _call("ipx_gram_shift", m, m_eq, None, _p(s_d), incs, _p(G))
    assert np.array_equal(G.cpu().numpy(), want)


@pytest.mark.parametrize("m_eq,m_in,n", [(7, 30, 301), (0, 64, 63), (100, 90, 1001)])
def test_structured_gram_vs_full_gram(m_eq, m_in, n):
    from ipsolver import dense
    from ipsolver.device import DVec
    rng = np.random.default_rng(n)
    Je, Ji = rng.standard_normal((m_eq, n)), rng.standard_normal((m_in, n))
    s = rng.uniform(1e-3, 3.0, m_in)
    m, N = m_eq + m_in, n + m_in
    from ipsolver import _hip
    M = int(_hip.load().ipx_dense_padded(m))
    st = types.SimpleNamespace(constant=False, gram0=None)
    A = dense.augment(cuda(Je).reshape(m_eq, n), cuda(Ji).reshape(m_in, n), DVec(cuda(s)),
                      n, m_eq, m_in, stack=st)
    assert isinstance(A, dense.AugmentedDense)
    from ipsolver.device import stream_ptr
    G = torch.empty((M, M), dtype=F64, device="cuda")
    dense.DenseNormalSolver._structured_gram(A, G, stream_ptr())
    Gf = torch.empty((M, M), dtype=F64, device="cuda")
    dense._gram(m, N, A.t, N, Gf, stream_ptr())
    g, gf = G.cpu().numpy(), Gf.cpu().numpy()
    d = np.sqrt(np.outer(np.diag(gf), np.diag(gf)))
    assert np.max(np.abs(g - gf) / d) <= 1e-14
    assert np.array_equal(g[m:, :], gf[m:, :]) and np.array_equal(g[:, m:], gf[:, m:])
    # a constant J keeps its Gram: the second factorization's G is the shift of the kept one
    st.constant = True
    G1 = torch.empty((M, M), dtype=F64, device="cuda")
    dense.DenseNormalSolver._structured_gram(A, G1, stream_ptr())
    assert st.gram0 is not None and np.array_equal(G1.cpu().numpy(), g)
    G2 = torch.empty((M, M), dtype=F64, device="cuda")
    dense.DenseNormalSolver._structured_gram(A, G2, stream_ptr())
    assert np.array_equal(G2.cpu().numpy(), g)


def test_host_callback_augmented_jacobian_is_the_vstack_form():
    """The numpy-callback path assembles on the device now: the same bits as the former
    np.vstack((np.hstack((J_eq, 0)), np.hstack((J_ineq, diag(s))))) upload, a plain DeviceDense
    (its normal matrix stays the Gram of the whole matrix)."""
    from ipsolver import backend_hip as bh
    from ipsolver.dense import AugmentedDense, DeviceDense
    from ipsolver.device import DVec
    rng = np.random.default_rng(5)
    for n_eq, n_ineq, n in ((3, 4, 11), (0, 6, 5), (20, 17, 301)):
        Je, Ji = rng.standard_normal((n_eq, n)), rng.standard_normal((n_ineq, n))
        s = DVec(cuda(rng.uniform(0.1, 2, n_ineq)))
        A = bh.augmented_jacobian(Je, Ji, s, n, n_eq, n_ineq)
        s_h = s.to_host()
        top = np.hstack((np.atleast_2d(Je).reshape(n_eq, n), np.zeros((n_eq, n_ineq))))
        bot = np.hstack((np.atleast_2d(Ji).reshape(n_ineq, n), np.diag(s_h)))
        want = np.vstack((top, bot))
        assert type(A) is DeviceDense and not isinstance(A, AugmentedDense)
        assert np.array_equal(A.t.cpu().numpy(), want)
        assert np.array_equal(A.T.t.cpu().numpy(), want.T)


# ---- refusals ------------------------------------------------------------------------------
def test_densified_rows_over_the_cap_are_refused():
    from ipsolver.dense import DenseNormalSolver
    n = DenseNormalSolver.MAX_ROWS_FROM_SPARSE + 1
    x0 = torch.zeros(n, dtype=F64, device="cuda")
    row = torch.ones((1, n), dtype=F64, device="cuda")
    cons = (ipsolver.LinearConstraint(row, ("less", 1.0)), ipsolver.BoxConstraint(("greater", -1.0)))
    with pytest.raises(NotImplementedError, match="MAX_ROWS_FROM_SPARSE"):
        ipsolver.minimize_constrained(lambda x: float(x.dot(x)), x0, lambda x: 2 * x,
                                      lambda x: 2 * torch.ones_like(x), cons)


def test_cpu_tensor_as_dense_linear_matrix_is_a_type_error():
    x0 = torch.zeros(3, dtype=F64, device="cuda")
    with pytest.raises(TypeError):
        ipsolver.minimize_constrained(lambda x: float(x.dot(x)), x0, lambda x: 2 * x,
                                      lambda x: 2 * torch.ones_like(x),
                                      ipsolver.LinearConstraint(torch.ones((1, 3), dtype=F64),
                                                                ("less", 1.0)))
