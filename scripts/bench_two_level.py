"""The preconditioners of the matrix-free (A A')^-1 (ipsolver/iterative.py, csrc/pcg.hip) against
each other on flow networks (tests/two_level_cases.py: A = [G, eps I], G the incidence matrix of an
N x N grid, so that A A' is a graph Laplacian plus eps^2): "block" (the yardstick: 32-row strips
of the reverse Cuthill-McKee order), "compact" (aggregate blocks) and "two-level" (aggregate
blocks plus the coarse correction).  Per size and preconditioner: iterations and milliseconds
per solve at the solver's own tolerance, milliseconds per factorization on a new pattern (with
the host graph work) and on a known one, split into row order / blocks / coarse level, storage,
and the true residual.  Times are host wall clock around work that ends in a device
synchronise; medians, with the smallest and largest beside them.

Every size runs in a child process of its own under a time limit; the first one that fails or
runs out of time ends the run.  The output goes to profiles/two_level_timings.txt as well.
    python scripts/bench_two_level.py [--quick]"""
import os, statistics, subprocess, sys, threading, time, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ip-nonlinear-solver_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

QUICK = "--quick" in sys.argv
# (N, eps, seconds allowed)
CASES = [(60, 0.1, 120), (120, 0.1, 120)] if QUICK else \
    [(316, 0.1, 240), (316, 0.01, 240), (700, 0.1, 480)]
PRECONDS = ("block", "compact", "two-level")


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


def split(solver):
    return ", ".join("%s %.3f" % (k, 1e3 * v) for k, v in solver.build_seconds.items())


def measure(N, eps):
    import numpy as np, torch
    import two_level_cases as tc
    from ipsolver import device as dv
    from ipsolver.iterative import IterativeNormalSolver
    sync = torch.cuda.synchronize
    A = tc.grid(N, eps)
    m, n = A.shape
    print("\n== grid N = %d, eps = %g: m = %d, n = %d, nnz = %d  (%s)"
          % (N, eps, m, n, A.nnz, torch.cuda.get_device_name(0)), flush=True)
    wh = tc.rhs(m)
    w = dv.DVec.from_host(wh)
    IterativeNormalSolver(dv.DeviceCSR.from_scipy(tc.grid(8)), precond="two-level").solve(
        dv.DVec.from_host(tc.rhs(64)))                 # warm: code objects, allocator
    sync()
    base = {}
    for precond in PRECONDS:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            Ad = dv.DeviceCSR.from_scipy(A)            # a pattern nothing is cached on
            sync()
            t0 = time.perf_counter()
            solver = IterativeNormalSolver(Ad, precond=precond)
            sync()
            first = 1e3 * (time.perf_counter() - t0)
            first_split = split(solver)
            made = []
            tf = wall(lambda: made.append(IterativeNormalSolver(Ad, precond=precond)), 3, sync)
            again_split = split(made[-1])
            del made[:]
            solver.solve(w)                            # warm
            before = dict(solver.stats)
            reps = 3
            ts = wall(lambda: solver.solve(w), reps, sync)
            x = solver.solve(w).to_host()
        st = solver.stats
        its = (st["iterations"] - before["iterations"]) / (reps + 1)
        res = np.linalg.norm(A @ (A.T @ x) - wh) / np.linalg.norm(wh)
        store = 8 * solver.binv.numel() + 4 * solver.border.numel()
        if precond == "two-level":
            store += 8 * solver.coarse.Ginv.t.numel() + 12 * solver.C.pattern.nnz + 4 * m
        print("  %-10s blocks %d, coarse rows %d (groups of <= %d blocks), storage %.1f MB"
              % (precond, st["blocks"], st["coarse_rows"], st["group"], 1e-6 * store))
        print("  %-10s solve %s, %.1f iterations, %.1f us per iteration, ||S x - w|| / ||w|| = "
              "%.2e%s" % ("", fmt(ts), its, 1e3 * ts[0] / max(its, 1), res,
                          "; warnings: " + "; ".join(sorted({str(c.message)[:80] for c in caught}))
                          if caught else ""))
        print("  %-10s factorization, new pattern %9.3f ms  [%s]" % ("", first, first_split))
        print("  %-10s factorization, known pattern %s  [%s]" % ("", fmt(tf), again_split))
        base[precond] = (ts[0], its, tf[0])
        if precond != "block":
            b = base["block"]
            print("  %-10s against \"block\": iterations x %.2f, solve time x %.2f, factorization "
                  "(known pattern) x %.2f" % ("", its / b[1], ts[0] / b[0], tf[0] / b[2]))
        sys.stdout.flush()
        del solver
        torch.cuda.empty_cache()


def main():
    if "--case" in sys.argv:
        k = sys.argv.index("--case")
        measure(int(sys.argv[k + 1]), float(sys.argv[k + 2]))
        return 0
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "two_level_timings.txt"), "w") as log:
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
