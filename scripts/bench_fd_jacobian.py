"""Finite-difference constraint Jacobians on the config-3 shape (dev tool): device callbacks,
n = 1e6 variables, m = 1e5 equality rows, tr_interior_point, with the analytic ``jac`` against
``jac='2-point'`` and ``'3-point'`` -- status, outer / CG iterations, ``jac_fd_nfev``, blocking
reads, wall clock of a warm solve --, and per Jacobian evaluation the time of the steps kernel,
the G perturb launches, the callbacks and the assemble (HIP events), with the three kernels'
algorithmic bytes and their share of 8 TB/s.

    python scripts/bench_fd_jacobian.py [--n N] [--max-iter K] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ip-nonlinear-solver_amd"))

import numpy as np
import scipy.sparse as sps
import torch

import ipsolver
from ipsolver import _hip
from ipsolver._numdiff import group_columns
from ipsolver.fd_jacobian import SparseFDPlan
from ipsolver.synthetic import CenteredBandedNLP, LeanDeviceCallbacks

PEAK_BYTES_PER_S = 8e12
COPY_SHARE = 0.79            # what a dwordx4 copy reaches on this part


def solve(dc, jac, max_iter, **kw):
    lib = _hip.load()
    con = ipsolver.NonlinearConstraint(dc.constr_fun, ("equals", 0), jac, dc.constr_hess, **kw)
    torch.cuda.synchronize()
    reads0 = lib.ipx_read_count()
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = ipsolver.minimize_constrained(dc.fun, dc.x0, dc.grad, dc.hess, con,
                                            method="tr_interior_point", max_iter=max_iter)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    row = {"status": int(res.status), "niter": int(res.niter), "cg_niter": int(res.cg_niter),
           "njev": int(res.njev), "blocking_reads": int(lib.ipx_read_count() - reads0),
           "wall_s": wall, "optimality": float(res.optimality),
           "constr_violation": float(res.constr_violation)}
    if "jac_fd_nfev" in res:
        row["jac_fd_nfev"] = int(res.jac_fd_nfev)
    return row


def timed(fn, reps):
    for _ in range(3):
        fn()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(reps):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) * 1e-3 / reps


def stages(dc, plan, method, reps=20):
    """Seconds per Jacobian evaluation of each stage, and the kernels' algorithmic bytes."""
    n, m, nnz, G = plan.n, plan.m, plan.nnz, plan.n_groups
    x = dc.x0
    f0 = dc.constr_fun(x)
    h, flags = plan.steps(x, method)
    dx = torch.empty(n, dtype=torch.float64, device=x.device)
    F1, F2 = plan._buffers(method)
    val = torch.empty(nnz, dtype=torch.float64, device=x.device)
    three = method == '3-point'
    points = [plan.perturb(x, h, flags, g, method, dx) for g in range(G)]

    def callbacks():
        for g, (x1, x2) in enumerate(points):
            F1[g].copy_(dc.constr_fun(x1))
            if three:
                F2[g].copy_(dc.constr_fun(x2))
    callbacks()
    t = {"steps_s": timed(lambda: plan.steps(x, method), reps),
         "perturb_s": timed(lambda: [plan.perturb(x, h, flags, g, method, dx) for g in range(G)],
                            reps),
         "callbacks_s": timed(callbacks, max(2, reps // 4)),
         "assemble_s": timed(lambda: plan.assemble(method, 0, G, f0, F1, F2, dx, flags, val), reps),
         "evaluate_s": timed(lambda: plan.evaluate(dc.constr_fun, x, method, f0=f0),
                             max(2, reps // 4))}
    # algorithmic bytes: steps reads x0, writes h and the flags; one perturb launch reads groups,
    # x0, h (and the flags for '3-point'), writes one or two points; the assemble reads col, writes
    # val, and gathers per entry groups / dx (/ flag) by column and f0 / F1 (/ F2) by row
    b = {"steps_bytes": 8 * n + 9 * n,
         "perturb_bytes": G * (4 * n + 16 * n + (n if three else 0) + (16 * n if three else 8 * n)),
         "assemble_bytes": nnz * (4 + 8 + 4 + 8 + 8 + 8 + (9 if three else 0))}
    for k in ("steps", "perturb", "assemble"):
        t[k + "_share_of_peak"] = b[k + "_bytes"] / t[k + "_s"] / PEAK_BYTES_PER_S
    t.update(b)
    t["assemble_share_vs_copy"] = t["assemble_share_of_peak"] / COPY_SHARE
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--max-iter", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_fd_jacobian_line.json"))
    args = ap.parse_args()
    n, m = args.n, args.n // 10
    prob = CenteredBandedNLP(n, m, eps=1e-3)
    dc = LeanDeviceCallbacks(prob)
    S = sps.csr_matrix((np.ones(prob.A0.nnz), prob.A0.indices, prob.A0.indptr),
                       shape=prob.A0.shape)
    t0 = time.perf_counter()
    groups = group_columns(S)
    out = {"n": n, "m": m, "nnz": int(S.nnz), "n_groups": int(groups.max()) + 1,
           "group_columns_s": time.perf_counter() - t0, "solves": {}, "stages": {}}
    sparsity = (S, groups)
    for name, jac, kw in (("analytic", dc.constr_jac, {}),
                          ("2-point", "2-point", {"finite_diff_jac_sparsity": sparsity}),
                          ("3-point", "3-point", {"finite_diff_jac_sparsity": sparsity})):
        solve(dc, jac, args.max_iter, **kw)                   # warm-up
        out["solves"][name] = solve(dc, jac, args.max_iter, **kw)
        print(name, out["solves"][name], flush=True)
    plan = SparseFDPlan(S, groups, n, m)
    for method in ("2-point", "3-point"):
        out["stages"][method] = stages(dc, plan, method)
        print(method, out["stages"][method], flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"fd_jacobian": out["solves"]}))


if __name__ == "__main__":
    main()
