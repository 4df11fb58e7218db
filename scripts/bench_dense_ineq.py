"""Dense constraint Jacobians with inequality rows in device-callback mode at BASELINE config 2's
size: ``DenseDeviceCallbacks.on_device(n, m)`` under ``synthetic.mixed_interval_kind(m)``
(a third equalities, a third one-sided, a third two-sided rows), solved to gtol with
``tr_interior_point`` as a NonlinearConstraint (a new dense Jacobian per step) and as a dense
LinearConstraint (constant J: the Gram is kept, one shift per refactorization), and the same
problem with numpy callbacks.  Prints ONE JSON line: status / counts / wall clock per solve,
HIP-event times of the assembly kernels (algorithmic bytes, fraction of 8 TB/s) and of the
factorization steps per refactorization.
    python scripts/bench_dense_ineq.py [n] [m] [--no-host]"""
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ip-nonlinear-solver_amd"))
import scipy.sparse as sps  # noqa: E402
import torch  # noqa: E402

import ipsolver  # noqa: E402
from ipsolver import _hip, dense, device as dv, device_mode as dm  # noqa: E402
from ipsolver.synthetic import CenteredDenseNLP, DenseDeviceCallbacks, mixed_interval_kind  # noqa: E402,E501

PEAK_GBS = 8000.0
args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 10000
m = int(args[1]) if len(args) > 1 else 2000
cb = DenseDeviceCallbacks.on_device(n, m)
kind = mixed_interval_kind(m)


def solve(constraints, fun=cb.fun, x0=cb.x0, grad=cb.grad, hess=cb.hess):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = ipsolver.minimize_constrained(fun, x0, grad, hess, constraints,
                                            method="tr_interior_point")
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return {"status": int(res.status), "niter": int(res.niter), "cg_niter": int(res.cg_niter),
            "njev": int(res.njev), "optimality": float(res.optimality),
            "constr_violation": float(res.constr_violation), "wall_clock_to_gtol_s": wall}


def timed(fn, reps=10):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


out = {"what": "dense Jacobian, mixed interval kind, device-callback mode", "n": n, "m": m}
nl = cb.constraints(ipsolver, kind)
lin = ipsolver.LinearConstraint(cb.A, kind)
small = DenseDeviceCallbacks(CenteredDenseNLP(300, 60))              # warm-up (code objects)
solve(small.constraints(ipsolver, mixed_interval_kind(60)), small.fun, small.x0, small.grad,
      small.hess)
out["nonlinear"] = solve(nl)
out["linear_constant_J"] = solve(lin)

# ---- the kernels on the problem's own shapes --------------------------------------------------
canon = dm.DeviceCanonical([nl], dv.DVec(cb.x0))
stack = canon.dense_stack
m_eq, m_in = stack.m_eq, stack.m_ineq
rows = m_eq + m_in
J = dense.DeviceDense(cb.constr_jac(cb.x0))
out["canonical_rows"] = {"eq": m_eq, "ineq": m_in}
k = {}
B = 8.0
t = timed(lambda: stack.assemble([J]))
k["gather_ms"] = t
k["gather_bytes"] = 2 * B * rows * n
k["gather_frac_of_8TBs"] = k["gather_bytes"] / (t * 1e-3) / 1e9 / PEAK_GBS
J_ineq, J_eq = stack.assemble([J])
s = dv.DVec(torch.rand(m_in, dtype=torch.float64, device="cuda") + 0.5)
N = n + m_in
A_buf = torch.empty((rows, N), dtype=torch.float64, device="cuda")
At_buf = torch.empty((N, rows), dtype=torch.float64, device="cuda")
t = timed(lambda: _hip.call("ipx_dense_augment", m_eq, m_in, n, dv._p(J_eq.t), n, dv._p(J_ineq.t),
                            n, dv._p(s.t), dv._p(A_buf), dv._p(At_buf), dv.stream_ptr()))
k["augment_ms"] = t
k["augment_bytes"] = B * (rows * n + m_in + 2 * rows * N)
k["augment_frac_of_8TBs"] = k["augment_bytes"] / (t * 1e-3) / 1e9 / PEAK_GBS
A = dense.augment(J_eq.t, J_ineq.t, s, n, m_eq, m_in, stack)
lib = _hip.load()
M = int(lib.ipx_dense_padded(rows))
st = dv.stream_ptr()
G = torch.empty((M, M), dtype=torch.float64, device="cuda")
G0 = torch.empty((M, M), dtype=torch.float64, device="cuda")
X = torch.empty((M, M), dtype=torch.float64, device="cuda")
flag = torch.zeros(1, dtype=torch.int32, device="cuda")
work = torch.zeros(M + 1, dtype=torch.float64, device="cuda")
s_ptr = A.t.data_ptr() + 8 * (m_eq * N + n)
k["gram_structured_ms"] = timed(lambda: dense._gram(rows, n, A.t, N, G0, st))
k["gram_full_width_ms"] = timed(lambda: dense._gram(rows, N, A.t, N, G, st))
t = timed(lambda: _hip.call("ipx_gram_shift", rows, m_eq, dv._p(G0), s_ptr, N + 1, dv._p(G), st))
k["shift_ms"] = t
k["shift_frac_of_8TBs"] = 2 * B * M * M / (t * 1e-3) / 1e9 / PEAK_GBS


def chol():
    _hip.call("ipx_gram_shift", rows, m_eq, dv._p(G0), s_ptr, N + 1, dv._p(G), st)
    _hip.call("ipx_chol_factor", M, dv._p(G), dv._p(flag), dv._p(work), st)


k["cholesky_ms"] = timed(chol) - k["shift_ms"]


def inverse():
    chol()
    _hip.call("ipx_chol_inverse", M, dv._p(G), dv._p(X), st)


k["inverse_ms"] = timed(inverse) - k["cholesky_ms"] - k["shift_ms"]
k["refactorization_ms"] = {"nonlinear": k["gram_structured_ms"] + k["shift_ms"] +
                           k["cholesky_ms"] + k["inverse_ms"],
                           "constant_J": k["shift_ms"] + k["cholesky_ms"] + k["inverse_ms"]}
out["kernels"] = k

# ---- numpy callbacks, the same problem -------------------------------------------------------
if "--no-host" not in sys.argv:
    A_h, W_h = cb.A.cpu().numpy(), cb.W.cpu().numpy()
    H_h = cb.H.cpu().numpy()
    H_h.setflags(write=False)
    q_h, xf_h, b_h = cb.q.cpu().numpy(), cb.x_feas.cpu().numpy(), cb.b.cpu().numpy()
    kap, eps = cb.p.kappa, cb.p.eps
    hst = solve(
        ipsolver.NonlinearConstraint(
            lambda x: A_h.dot(x) + 0.5 * kap * W_h.dot(x * x) - b_h, kind,
            lambda x: A_h + kap * W_h * x[None, :],
            lambda x, v: sps.diags(kap * W_h.T.dot(v), format="csr")),
        fun=lambda x: 0.5 * (x - xf_h).dot(H_h.dot(x - xf_h)) - eps * q_h.dot(x - xf_h),
        x0=cb.x0.cpu().numpy(), grad=lambda x: H_h.dot(x - xf_h) - eps * q_h,
        hess=lambda x: H_h)
    out["numpy_callbacks"] = hst
print(json.dumps(out))
