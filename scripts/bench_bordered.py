"""The bordered direct (A A')^-1 (csrc/bordered.hip) on the matrices of DESIGN.md section 4i: staged
dynamics (tests/blocktri_cases.ocp_rows, d = 8 and 16) and a tridiagonal A A' at m ~ 1e5 with
p = 1, 4, 32 dense columns, and one staged matrix at the dense solver's limit with p = 4 --
against the preconditioned CG and, while it fits, the dense Cholesky.
Times are host wall clock around work that ends in a device synchronise, the symbolic analysis
(cached on the pattern) excluded; medians, with the smallest and largest beside them.

The selection without the option starts with the symbolic analysis of the full pattern, and with
one dense column A A' is full: 2.7e8 entries at m = 16384 and 1e10 at m = 1e5, on the host.  It is
not run here; the CG is measured with its diagonal preconditioner, which needs no analysis (its
block preconditioner takes its row order from that analysis).
    python scripts/bench_bordered.py [--quick]"""
import os, statistics, sys, time, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ip-nonlinear-solver_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import blocktri_cases as bc
import bordered_cases as bd
from ipsolver import _hip, device as dv, projector
from ipsolver.bordered import BorderedNormalSolver, border_split
from ipsolver.dense import DenseNormalSolver

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


def measure(name, base, p, reach):
    rng = np.random.default_rng(p)
    A, cols = bd.bordered(rng, base, p, 1.0, int(np.abs(base.data).max()))
    m, n = A.shape
    Ad = dv.DeviceCSR.from_scipy(A)
    t0 = time.perf_counter()
    split = border_split(Ad.pattern, reach, p)
    assert split is not None and split.p == p
    print("\n== %s + %d dense columns: m = %d, n = %d, nnz = %d, band half bandwidth %d (pattern "
          "analysis %.2f s, host, once per pattern)"
          % (name, p, m, n, A.nnz, split.k, time.perf_counter() - t0), flush=True)
    w = dv.DVec.from_host(np.random.default_rng(1).standard_normal(m))
    small = m <= DenseNormalSolver.MAX_ROWS_FROM_SPARSE
    kinds = [("bordered", lambda: BorderedNormalSolver(Ad, split), 5, 20),
             ("preconditioned CG", lambda: projector.IterativeNormalSolver(Ad, precond="jacobi"),
              3, 5)]
    if small:
        kinds.append(("dense Cholesky", lambda: DenseNormalSolver(Ad), 2, 20))
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
        print("  %-18s factorization %s   solve %s" % (label, fmt(tf), fmt(ts)))
        if label == "bordered":
            print("  %-18s inner %s (k = %d), trace(K) = %.3g, refinement %s, partial blocks %d, "
                  "ws %.1f MB" % ("", type(solver.inner).__name__, solver.inner.k, solver.growth,
                                  "on" if solver.refine else "off", solver.groups,
                                  8e-6 * solver.ws.numel()))
        elif label == "preconditioned CG":
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
    wh, ref = w.to_host(), xs["bordered"]
    for label, x in xs.items():
        r = A @ (A.T @ x) - wh
        print("  %-18s ||S x - w|| / ||w|| = %.2e, ||x - x_bordered|| / ||x_bordered|| = %.2e"
              % (label, np.linalg.norm(r) / np.linalg.norm(wh),
                 np.linalg.norm(x - ref) / np.linalg.norm(ref)))
    sys.stdout.flush()


print("device: %s; torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
scale = 20 if QUICK else 1
rng = np.random.default_rng(0)
lib = _hip.load()
m5 = 100000 // scale
for p in (1, 4, 32):
    for d in (8, 16):
        measure("ocp_rows(d = %d, c = %d, stages = %d)" % (d, d // 4, -(-m5 // d)),
                bc.ocp_rows(d, d // 4, -(-m5 // d), rng), p, lib.ipx_blocktri_kmax())
    measure("tridiagonal band_rows(m = %d, k = 1)" % m5, bc.band_rows(rng, m5, 1, lim=2 ** 4), p,
            lib.ipx_banded_kmax())
measure("ocp_rows(d = 16, c = 4, stages = %d) -- the dense solver's limit" % (1024 // scale),
        bc.ocp_rows(16, 4, 1024 // scale, rng), 4, lib.ipx_blocktri_kmax())
