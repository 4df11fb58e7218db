"""The nested-dissection direct (A A')^-1 (ipsolver/nested.py, csrc/nested.hip) against the
matrix-free one (ipsolver/iterative.py) under its "block" and "two-level" preconditioners, in the
same run, on flow networks (tests/two_level_cases.py: A = [G, eps I], G the incidence matrix of an
N x N grid, so that A A' is a graph Laplacian plus eps^2).  Per size and solver: milliseconds and
launches per solve, milliseconds per factorization on a new pattern (with the host graph work; for
the direct solver the host time of the analysis alone beside it) and on a known one, storage, and
the true residual ||S x - w|| / ||w||.  Times are host wall clock around work that ends in a
device synchronise; medians of REPS runs after a warm-up run, the smallest and largest beside
them.

Every size runs in a child process of its own under a time limit; the first one that fails or
runs out of time ends the run.  The output goes to profiles/nested_dissection_timings.txt as well.
    python scripts/bench_nested_dissection.py [--quick]"""
import os, statistics, subprocess, sys, threading, time, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ip-nonlinear-solver_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

QUICK = "--quick" in sys.argv
# (N, eps, seconds allowed)
CASES = [(60, 0.1, 120), (120, 0.01, 120)] if QUICK else \
    [(316, 0.1, 240), (316, 0.01, 240), (700, 0.1, 480)]
REPS = 7


def wall(fn, reps, sync):
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


def measure(N, eps):
    import numpy as np, torch
    import two_level_cases as tc
    from ipsolver import _hip, device as dv
    from ipsolver.iterative import IterativeNormalSolver
    from ipsolver.nested import NestedDissectionNormalSolver
    sync = torch.cuda.synchronize
    lib = _hip.load()
    A = tc.grid(N, eps)
    m, n = A.shape
    print("\n== grid N = %d, eps = %g: m = %d, n = %d, nnz = %d  (%s)"
          % (N, eps, m, n, A.nnz, torch.cuda.get_device_name(0)), flush=True)
    wh = tc.rhs(m)
    w = dv.DVec.from_host(wh)
    small = dv.DeviceCSR.from_scipy(tc.grid(20))       # warm: code objects, allocator
    for warm in (NestedDissectionNormalSolver(small),
                 IterativeNormalSolver(small, precond="two-level")):
        warm.solve(dv.DVec.from_host(tc.rhs(400)))
    sync()
    makers = (("nested-dissection", NestedDissectionNormalSolver),
              ("block", lambda Ad: IterativeNormalSolver(Ad, precond="block")),
              ("two-level", lambda Ad: IterativeNormalSolver(Ad, precond="two-level")))
    base = {}
    for name, make in makers:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            Ad = dv.DeviceCSR.from_scipy(A)            # a pattern nothing is cached on
            sync()
            t0 = time.perf_counter()
            solver = make(Ad)
            sync()
            first = 1e3 * (time.perf_counter() - t0)
            made = []
            tf = wall(lambda: made.append(make(Ad)), 3, sync)
            del made[:]
            solver.solve(w)                            # warm
            before = lib.ipx_launch_count()
            ts = wall(lambda: solver.solve(w), REPS, sync)
            launches = (lib.ipx_launch_count() - before) / REPS
            x = solver.solve(w).to_host()
        res = np.linalg.norm(A @ (A.T @ x) - wh) / np.linalg.norm(wh)
        st = solver.stats
        if name == "nested-dissection":
            store = st["storage_bytes"]
            print("  %-18s %d fronts (%d tiled, largest %d), %d tree levels, factor %.1f MB, "
                  "storage %.1f MB" % (name, st["fronts"], st["large_fronts"], st["largest_front"],
                                       st["levels"], 1e-6 * st["factor_bytes"], 1e-6 * store))
            extra = "host analysis alone %.3f ms" % (1e3 * solver.analysis_seconds)
        else:
            store = 8 * solver.binv.numel() + 4 * solver.border.numel()
            if name == "two-level":
                store += 8 * solver.coarse.Ginv.t.numel() + 12 * solver.C.pattern.nnz + 4 * m
            print("  %-18s blocks %d, coarse rows %d, storage %.1f MB"
                  % (name, st["blocks"], st["coarse_rows"], 1e-6 * store))
            extra = "%.1f iterations per solve" % (st["iterations"] / st["solves"])
        print("  %-18s solve %s, %.1f launches, ||S x - w|| / ||w|| = %.2e%s"
              % ("", fmt(ts), launches, res,
                 "; warnings: " + "; ".join(sorted({str(c.message)[:80] for c in caught}))
                 if caught else ""))
        print("  %-18s factorization, new pattern %9.3f ms  [%s]" % ("", first, extra))
        print("  %-18s factorization, known pattern %s" % ("", fmt(tf)))
        base[name] = (ts[0], tf[0])
        if name != "nested-dissection":
            d = base["nested-dissection"]
            gain = base[name][0] - d[0]
            pays = "never" if gain <= 0 else \
                "from the first solve on" if d[1] <= base[name][1] else \
                "after %.0f solves" % np.ceil((d[1] - base[name][1]) / gain)
            print("  %-18s nested dissection against this: solve time x %.3f, factorization "
                  "(known pattern) x %.2f; pays %s" % ("", d[0] / base[name][0],
                                                       d[1] / base[name][1], pays))
        sys.stdout.flush()
        del solver
        torch.cuda.empty_cache()


def main():
    if "--case" in sys.argv:
        k = sys.argv.index("--case")
        measure(int(sys.argv[k + 1]), float(sys.argv[k + 2]))
        return 0
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    name = "nested_dissection_timings%s.txt" % ("_quick" if QUICK else "")
    with open(os.path.join(ROOT, "profiles", name), "w") as log:
        for N, eps, limit in CASES:
            proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--case", str(N),
                                     str(eps)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                    text=True)
            timer = threading.Timer(limit, proc.kill)
            timer.start()
            for line in proc.stdout:
                sys.stdout.write(line)
                sys.stdout.flush()
                log.write(line)
                log.flush()
            rc = proc.wait()
            timer.cancel()
            if rc != 0:
                print("N = %d, eps = %g ended with status %d: stopping here" % (N, eps, rc))
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
