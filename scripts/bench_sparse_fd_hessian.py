"""Sparse finite-difference Hessians on the config-3 shape (dev tool): lean device callbacks,
n = 1e6 variables, m = 1e5 equality rows, tr_interior_point, with the exact Hessians against the
operator form ``hess='2-point'`` and ``hess=SparseFD('2-point')`` (objective and constraint) --
status, outer / CG iterations, ``ngev``, ``hess_fd_ngev``, blocking reads, wall clock of a warm
solve --, and per Hessian evaluation of the objective's term the time of the steps kernel, the
G perturb launches, the gradient calls and the symmetric assemble (HIP events), with the
assemble's algorithmic bytes and its share of 8 TB/s.

    python scripts/bench_sparse_fd_hessian.py [--n N] [--max-iter K] [--out FILE.json]
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
from ipsolver.fd_hessian import SparseFDHessianPlan
from ipsolver.synthetic import CenteredBandedNLP, LeanDeviceCallbacks

PEAK_BYTES_PER_S = 8e12


def solve(dc, hess, constr_hess, max_iter):
    lib = _hip.load()
    con = ipsolver.NonlinearConstraint(dc.constr_fun, ("equals", 0), dc.constr_jac, constr_hess)
    calls = [0]

    def grad(x):
        calls[0] += 1
        return dc.grad(x)
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
           "ngev": int(res.ngev), "gradient_calls": calls[0],
           "blocking_reads": int(lib.ipx_read_count() - reads0), "wall_s": wall,
           "optimality": float(res.optimality), "constr_violation": float(res.constr_violation)}
    for k in ("hess_fd_ngev", "hess_fd_njev"):
        if k in res:
            row[k] = int(res[k])
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
    """Seconds per Hessian evaluation of each stage, and the assemble's algorithmic bytes."""
    n, nnz, G = plan.n, plan.nnz, plan.n_groups
    x = dc.x0
    f0 = dc.grad(x)
    h, flags = plan.steps(x, method)
    dx = torch.empty(n, dtype=torch.float64, device=x.device)
    F1, F2 = plan._buffers(method)
    val = torch.empty(nnz, dtype=torch.float64, device=x.device)
    three = method == '3-point'
    points = [plan.perturb(x, h, flags, g, method, dx) for g in range(G)]

    def callbacks():
        for g, (x1, x2) in enumerate(points):
            F1[g].copy_(dc.grad(x1))
            if three:
                F2[g].copy_(dc.grad(x2))
    callbacks()
    t = {"steps_s": timed(lambda: plan.steps(x, method), reps),
         "perturb_s": timed(lambda: [plan.perturb(x, h, flags, g, method, dx) for g in range(G)],
                            reps),
         "callbacks_s": timed(callbacks, max(2, reps // 4)),
         "assemble_s": timed(lambda: plan.assemble_sym(method, 0, G, f0, F1, F2, dx, flags, val),
                             reps),
         "evaluate_s": timed(lambda: plan.evaluate(dc.grad, x, method, f0=f0), max(2, reps // 4))}
    # algorithmic bytes of the symmetric assemble: col in, val out, and per entry the gathers of
    # both halves: groups / dx (/ flag) by column and by row, f0 by row and by column, F1 (/ F2)
    # at (group of the column, row) and (group of the row, column)
    t["assemble_bytes"] = nnz * (4 + 8 + 2 * (4 + 8 + 8 + 8) + (2 * 9 if three else 0))
    t["assemble_share_of_peak"] = t["assemble_bytes"] / t["assemble_s"] / PEAK_BYTES_PER_S
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--max-iter", type=int, default=1000)
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "r10_sparse_fd_hessian_line.json"))
    args = ap.parse_args()
    n, m = args.n, args.n // 10
    prob = CenteredBandedNLP(n, m, eps=1e-3)
    dc = LeanDeviceCallbacks(prob)
    Sf = sps.csr_matrix((np.ones(prob.Q.nnz), prob.Q.indices, prob.Q.indptr), shape=prob.Q.shape)
    # the tridiagonal pattern's optimal grouping is column mod 3 (group_columns is greedy along
    # a random order and finds more groups)
    gf = (np.arange(n) % 3).astype(np.int32)
    Sc, gc = sps.identity(n, format="csr"), np.zeros(n, dtype=np.int32)
    out = {"n": n, "m": m, "nnz": int(Sf.nnz), "n_groups_objective": 3,
           "n_groups_objective_greedy": int(group_columns(Sf).max()) + 1,
           "n_groups_constraint": 1, "solves": {}, "stages": {}}
    sfd = lambda: (ipsolver.SparseFD('2-point', Sf, gf), ipsolver.SparseFD('2-point', Sc, gc))
    for name, make in (("exact", lambda: (dc.hess, dc.constr_hess)),
                       ("2-point operator", lambda: ('2-point', '2-point')),
                       ("SparseFD 2-point", sfd)):
        solve(dc, *make(), args.max_iter)                     # warm-up
        out["solves"][name] = solve(dc, *make(), args.max_iter)
        print(name, out["solves"][name], flush=True)
    plan = SparseFDHessianPlan(Sf, gf, n)
    for method in ("2-point", "3-point"):
        out["stages"][method] = stages(dc, plan, method)
        print(method, out["stages"][method], flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"sparse_fd_hessian": out["solves"]}))


if __name__ == "__main__":
    main()
