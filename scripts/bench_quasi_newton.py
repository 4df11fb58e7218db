"""Quasi-Newton Hessians on the config-3 shape (dev tool): device callbacks, n = 1e6 variables,
m = 1e5 equality rows, tr_interior_point, with the exact Hessian, hess='2-point', LBFGS(5) and
LSR1(5) -- status, outer / CG iterations, gradient calls, blocking reads, wall clock of a warm
solve --, the quasi-Newton solves once more with the term applied by the host between the CG
iterations (IPX_DEBUG_FORMS=no-lowrank-loop) for the CG iterations/s of the two forms, and the
stand-alone product / update timed with HIP events.  The in-loop kernels' durations come from a
kernel trace of this script (rocprofv3 --kernel-trace --stats -- python ... --only LBFGS(5)).

    python scripts/bench_quasi_newton.py [--n N] [--max-iter K] [--only NAME] [--out FILE.json]
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
import torch

import ipsolver
from ipsolver import _hip
from ipsolver.synthetic import CenteredBandedNLP, DeviceCallbacks

PEAK_BYTES_PER_S = 8e12


class Counted:
    def __init__(self, f):
        self.f, self.calls = f, 0

    def __call__(self, *a):
        self.calls += 1
        return self.f(*a)


def solve(dc, hess, max_iter):
    lib = _hip.load()
    grad = Counted(dc.grad)
    torch.cuda.synchronize()
    reads0 = lib.ipx_read_count()
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = ipsolver.minimize_constrained(dc.fun, dc.x0, grad, hess, dc.constraints(ipsolver),
                                            method="tr_interior_point", max_iter=max_iter)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    row = {"status": int(res.status), "niter": int(res.niter), "cg_niter": int(res.cg_niter),
           "grad_calls": grad.calls, "ngev": int(res.ngev),
           "blocking_reads": int(lib.ipx_read_count() - reads0), "wall_s": wall,
           "cg_iter_per_s": res.cg_niter / wall, "optimality": float(res.optimality),
           "constr_violation": float(res.constr_violation)}
    if "hess_updates" in res:
        row["hess_updates"], row["hess_skipped"] = int(res.hess_updates), int(res.hess_skipped)
    return row


def product_line(n, memory, reps=200):
    """ipx_lowrank_apply (two kernels) on a full memory: time per product and the share of
    8 TB/s its algorithmic bytes reach -- W twice (the partial sums, then out = sigma p + W c),
    p twice, out once: (2r + 3) 8n bytes, r = 2 memory."""
    from ipsolver import quasi_newton as qn
    from ipsolver.device import DVec, _p, stream_ptr
    rng = np.random.default_rng(0)
    mem = qn._Memory(ipsolver.LBFGS(memory), n)
    d = DVec.from_host(rng.uniform(1.0, 10.0, n))
    for _ in range(memory + 1):
        s = DVec.from_host(rng.standard_normal(n))
        y = d * s
        _hip.call("ipx_lowrank_update", 0, n, memory, 0.0, 1e-8, _p(mem.W), _p(s.t), _p(y.t),
                  _p(mem.state), _p(mem.part), stream_ptr())
    p = DVec.from_host(rng.standard_normal(n))
    out = DVec.zeros(n)
    for _ in range(10):
        mem.term.dot(p, out=out)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(reps):
        mem.term.dot(p, out=out)
    ev1.record()
    torch.cuda.synchronize()
    t_prod = ev0.elapsed_time(ev1) * 1e-3 / reps
    s = DVec.from_host(rng.standard_normal(n))
    y = d * s
    ev0.record()
    for _ in range(reps):
        _hip.call("ipx_lowrank_update", 0, n, memory, 0.0, 1e-8, _p(mem.W), _p(s.t), _p(y.t),
                  _p(mem.state), _p(mem.part), stream_ptr())
    ev1.record()
    torch.cuda.synchronize()
    t_upd = ev0.elapsed_time(ev1) * 1e-3 / reps
    r = 2 * memory
    nbytes = (2 * r + 3) * 8 * n
    return {"memory": memory, "r": r, "n": n, "product_us": 1e6 * t_prod,
            "product_bytes": nbytes, "product_share_of_8TBps": nbytes / t_prod / PEAK_BYTES_PER_S,
            "update_us": 1e6 * t_upd,
            "update_bytes": (2 * r + 2) * 8 * n + 4 * 8 * n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--max-iter", type=int, default=1000)
    ap.add_argument("--skip-solves", action="store_true")
    ap.add_argument("--skip-products", action="store_true")
    ap.add_argument("--only", default=None, help="one variant: exact, 2-point, LBFGS(5), LSR1(5)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    line = {"n": args.n, "m": args.n // 10}
    if not args.skip_products:
        line["products"] = [product_line(args.n, k) for k in (5, 10)]
        print(json.dumps(line["products"]), flush=True)
    if not args.skip_solves:
        dc = DeviceCallbacks(CenteredBandedNLP(args.n, args.n // 10, eps=1e-3))
        variants = [("exact", lambda: dc.hess), ("2-point", lambda: "2-point"),
                    ("LBFGS(5)", lambda: ipsolver.LBFGS(5)), ("LSR1(5)", lambda: ipsolver.LSR1(5))]
        line["solves"] = {}
        for name, h in variants:
            if args.only and name != args.only:
                continue
            solve(dc, h(), args.max_iter)                 # warm
            line["solves"][name] = row = solve(dc, h(), args.max_iter)
            print(name, json.dumps(row), flush=True)
            if name.startswith("L") and not args.only:
                # the same solve with the term applied by the host between the iterations
                os.environ["IPX_DEBUG_FORMS"] = "no-lowrank-loop"
                try:
                    solve(dc, h(), args.max_iter)
                    row = solve(dc, h(), args.max_iter)
                finally:
                    del os.environ["IPX_DEBUG_FORMS"]
                line["solves"][name + " no-lowrank-loop"] = row
                print(name, "no-lowrank-loop", json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(line, f, indent=1)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
