"""The linked direct (A A')^-1 (csrc/linked.hip) on the matrices of DESIGN.md section 4j: staged
dynamics (tests/blocktri_cases.ocp_rows, d = 8 and 16) and a tridiagonal A A' at m ~ 1e5 with
q = 1, 4, 32 full link rows -- against the preconditioned CG (the dense Cholesky cannot run at
that size).  Times are host wall clock around work that ends in a device synchronise, the pattern
analysis (cached on the pattern) apart; medians, with the smallest and largest beside them.

The selection without the option starts with the symbolic analysis of the full pattern, and with
one dense row A A' has a full row and column: on the host, with fill that buys nothing.  It is not
run here; the CG is measured with its diagonal preconditioner, which needs no analysis (its block
preconditioner takes its row order from that analysis).
    python scripts/bench_link_rows.py [--quick]"""
import os, statistics, sys, time, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ip-nonlinear-solver_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import blocktri_cases as bc
import link_cases as lc
from ipsolver import _hip, device as dv, projector
from ipsolver.linked import LinkedRowsNormalSolver, link_split

QUICK = "--quick" in sys.argv
sync = torch.cuda.synchronize


def wall(fn, reps):
    """(median, min, max) in ms of fn() followed by a synchronise."""
    out = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(out), min(out), max(out)


def fmt(t):
    return "%9.3f ms (%.3f .. %.3f)" % t


def measure(name, base, q, reach):
    rng = np.random.default_rng(q)
    A, rows = lc.linked(rng, base, q, 1.0, int(np.abs(base.data).max()), "bottom")
    m, n = A.shape
    Ad = dv.DeviceCSR.from_scipy(A)
    t0 = time.perf_counter()
    split = link_split(Ad.pattern, reach, q)
    assert split is not None and np.array_equal(split.d_rows, rows)
    print("\n== %s + %d full link rows: m = %d, n = %d, nnz = %d, band half bandwidth %d (pattern "
          "analysis %.2f s, host, once per pattern)"
          % (name, q, m, n, A.nnz, split.k, time.perf_counter() - t0), flush=True)
    w = dv.DVec.from_host(np.random.default_rng(1).standard_normal(m))
    kinds = [("linked", lambda: LinkedRowsNormalSolver(Ad, split), 5, 20),
             ("preconditioned CG", lambda: projector.IterativeNormalSolver(Ad, precond="jacobi"),
              3, 5)]
    xs = {}
    for label, make, nf, ns in kinds:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            solver = make()                                    # warm: code objects, allocator
            solver.solve(w)
            sync()
            tf = wall(make, 1 if QUICK else nf)
            solver = make()
            before = dict(solver.stats) if hasattr(solver, "stats") else {}
            ts = wall(lambda: solver.solve(w), 2 if QUICK else ns)
            x = solver.solve(w)
            sync()
        xs[label] = x.to_host()
        print("  %-18s factorization %s   solve %s" % (label, fmt(tf), fmt(ts)), flush=True)
        if label == "linked":
            print("  %-18s inner %s (k = %d), max F_jj / K_jj = %.3g, pivot bits %d, partial "
                  "blocks %d, ws %.1f MB (D' %.1f MB)"
                  % ("", type(solver.inner).__name__, solver.inner.k, solver.cancellation,
                     solver.flag_bits, solver.groups, 8e-6 * solver.ws.numel(),
                     8e-6 * solver.Dt.numel()))
        else:
            st = solver.stats
            done = max(st["solves"] - before.get("solves", 0), 1)
            print("  %-18s %s preconditioner, inner iterations per solve %.1f, blocking reads per "
                  "solve %.1f%s"
                  % ("", solver.precond, (st["iterations"] - before.get("iterations", 0)) / done,
                     (st["batches"] - before.get("batches", 0)) / done,
                     "; warnings: " + "; ".join(sorted({str(c.message)[:90] for c in caught}))
                     if caught else ""))
        del solver
        torch.cuda.empty_cache()
    wh, ref = w.to_host(), xs["linked"]
    for label, x in xs.items():
        r = A @ (A.T @ x) - wh
        print("  %-18s ||S x - w|| / ||w|| = %.2e, ||x - x_linked|| / ||x_linked|| = %.2e"
              % (label, np.linalg.norm(r) / np.linalg.norm(wh),
                 np.linalg.norm(x - ref) / np.linalg.norm(ref)))
    sys.stdout.flush()


print("device: %s; torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
scale = 20 if QUICK else 1
rng = np.random.default_rng(0)
lib = _hip.load()
m5 = 100000 // scale
with projector.wide_band("block-tridiagonal"):
    for q in (1, 4, 32):
        for d in (8, 16):
            measure("ocp_rows(d = %d, c = %d, stages = %d)" % (d, d // 4, -(-m5 // d)),
                    bc.ocp_rows(d, d // 4, -(-m5 // d), rng), q, lib.ipx_blocktri_kmax())
        measure("tridiagonal band_rows(m = %d, k = 1)" % m5, bc.band_rows(rng, m5, 1, lim=2 ** 4),
                q, lib.ipx_banded_kmax())
