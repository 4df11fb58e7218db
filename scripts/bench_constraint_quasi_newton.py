"""Quasi-Newton Hessians on a nonlinear constraint, config-3 shape (dev tool): lean device
callbacks, n = 1e6 variables, m = 1e5 equality rows, tr_interior_point.  Rows: exact Hessians;
``hess='2-point'`` on the constraint (the operator form); ``LSR1(5)`` on the constraint with the
objective exact; ``LSR1(5)`` on both.  Per row: status, outer / CG iterations, Jacobian and
gradient calls, blocking reads, wall clock of a warm solve.  Then the kernel that forms the pair's
y (``ipx_csr_tdiff_dot``) on the constraint's pattern, timed with HIP events: time per launch,
algorithmic bytes and their share of 8 TB/s.

    python scripts/bench_constraint_quasi_newton.py [--n N] [--max-iter K] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ip-nonlinear-solver_amd"))

import torch

import ipsolver
from ipsolver import _hip
from ipsolver import quasi_newton as qn
from ipsolver.synthetic import CenteredBandedNLP, LeanDeviceCallbacks

PEAK_BYTES_PER_S = 8e12


class Counted:
    def __init__(self, f):
        self.f, self.calls = f, 0

    def __call__(self, *a):
        self.calls += 1
        return self.f(*a)


def solve(dc, hess, constr_hess, max_iter):
    lib = _hip.load()
    grad, jac = Counted(dc.grad), Counted(dc.constr_jac)
    con = ipsolver.NonlinearConstraint(dc.constr_fun, ("equals", 0), jac, constr_hess)
    torch.cuda.synchronize()
    reads0 = lib.ipx_read_count()
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = ipsolver.minimize_constrained(dc.fun, dc.x0, grad, hess, con,
                                            method="tr_interior_point", max_iter=max_iter)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    row = {"status": int(res.status), "niter": int(res.niter), "cg_niter": int(res.cg_niter),
           "njev": int(res.njev), "jacobian_calls": jac.calls, "ngev": int(res.ngev),
           "gradient_calls": grad.calls, "blocking_reads": int(lib.ipx_read_count() - reads0),
           "wall_s": wall, "optimality": float(res.optimality),
           "constr_violation": float(res.constr_violation)}
    if "hess_updates" in res:
        row["hess_updates"], row["hess_skipped"] = int(res.hess_updates), int(res.hess_skipped)
    return row


def y_kernel(dc, reps=200):
    """One launch of ipx_csr_tdiff_dot with the gradients fused, on the constraint's pattern."""
    x0 = dc.x0
    x1 = x0 + 1e-3
    J0, J1 = dc.constr_jac(x0), dc.constr_jac(x1)
    g0, g1 = dc.grad(x0).clone(), dc.grad(x1).clone()
    pat = J0.pattern
    m, n = pat.shape
    v = torch.ones(m, dtype=torch.float64, device=x0.device)
    y = torch.empty(n, dtype=torch.float64, device=x0.device)
    fn = lambda: qn.tdiff_dot(pat, J1.val, J0.val, v, y, base=(g1, g0))
    for _ in range(5):
        fn()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(reps):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    t = ev0.elapsed_time(ev1) * 1e-3 / reps
    # per entry: row index 4, permutation 8, two values 16, the gathered multiplier 8; per
    # variable: a row pointer 4, y out 8, the two gradients 16
    nbytes = 36 * pat.nnz + 28 * n
    return {"n": n, "m": m, "nnz": pat.nnz, "launch_us": 1e6 * t, "bytes": nbytes,
            "share_of_8TBps": nbytes / t / PEAK_BYTES_PER_S}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--max-iter", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                  "r11_constraint_quasi_newton_line.json"))
    args = ap.parse_args()
    n, m = args.n, args.n // 10
    dc = LeanDeviceCallbacks(CenteredBandedNLP(n, m, eps=1e-3))
    out = {"n": n, "m": m, "solves": {}}
    rows = (("exact", lambda: (dc.hess, dc.constr_hess)),
            ("constraint 2-point", lambda: (dc.hess, '2-point')),
            ("constraint LSR1(5), objective exact", lambda: (dc.hess, ipsolver.LSR1(5))),
            ("LSR1(5) on both", lambda: (ipsolver.LSR1(5), ipsolver.LSR1(5))))
    for name, make in rows:
        solve(dc, *make(), args.max_iter)                     # warm-up
        out["solves"][name] = solve(dc, *make(), args.max_iter)
        print(name, json.dumps(out["solves"][name]), flush=True)
    out["y_kernel"] = y_kernel(dc)
    print("y kernel", json.dumps(out["y_kernel"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"constraint_quasi_newton": out["solves"]}))


if __name__ == "__main__":
    main()
