"""The device exit for rank-deficient sparse Jacobians (``sparse_rank_deficient = "skip-pivots"``:
ipsolver/sparse_deficient.py, the skip mode of csrc/nested.hip) on flow networks
(tests/two_level_cases.py: A = [G, 2^-3 I] of an N x N grid) with q duplicated rows appended:

  * per size and q: the pivot-skipping factorization alone, the whole projector (that
    factorization, q solves, the q x q Woodbury pieces, the dependency residual) and Z, LS, Y,
    against the full-rank nested-dissection solver and its normal-equation operators on the matrix
    WITHOUT those rows; at N = 48 also against the host exit (``SVDProjector``);
  * ``--untouched [--lib PATH]``: the two paths the change must leave alone -- the normal-mode
    nested factorization and the dense Cholesky ``ipx_chol_factor`` (the refactorization of the
    dense benchmark) -- with the library at PATH (a build of the parent commit) or this tree's.
    Run it alternating between the two builds and compare medians with the run-to-run spread.

Times are host wall clock around work that ends in a device synchronise: medians of REPS calls
after a warm-up call, the smallest and largest beside them.
    python scripts/bench_sparse_rank_deficient.py [--quick] | --untouched [--lib PATH]"""
import os, statistics, sys, time, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ip-nonlinear-solver_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

QUICK = "--quick" in sys.argv
SIZES = (48, 100) if QUICK else (48, 100, 700)
DROPPED = (1, 8, 32)
REPS = 7


def wall(fn, sync, reps=REPS):
    """(median, min, max) in ms of fn() followed by a synchronise, after one warm-up call."""
    fn()
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


def with_duplicates(A, q):
    """A and q copies of rows spread over it, appended."""
    import numpy as np, scipy.sparse as sps
    m = A.shape[0]
    rows = [(k + 1) * m // (q + 1) for k in range(q)]
    out = sps.vstack([A] + [A[i] for i in rows], format="csr")
    out.sort_indices()
    return out, np.arange(m, m + q)


def operators(P, n, m, sync):
    import numpy as np
    from ipsolver import device as dv
    rng = np.random.default_rng(0)
    x, b = dv.DVec.from_host(rng.standard_normal(n)), dv.DVec.from_host(rng.standard_normal(m))
    return [("Z", wall(lambda: P.null_space(x), sync)), ("LS", wall(lambda: P.least_squares(x), sync)),
            ("Y", wall(lambda: P.row_space(b), sync))]


def measure(N):
    import numpy as np, torch
    import two_level_cases as tc
    from ipsolver import device as dv, projector
    from ipsolver.nested import NestedDissectionNormalSolver, PivotSkippingNestedSolver
    from ipsolver.sparse_deficient import SparseDeficientProjector
    sync = torch.cuda.synchronize
    A0 = tc.grid(N, 0.125)
    m0, n = A0.shape
    print("\n== grid N = %d: m = %d, n = %d, nnz = %d  (%s)"
          % (N, m0, n, A0.nnz, torch.cuda.get_device_name(0)), flush=True)
    A0d = dv.DeviceCSR.from_scipy(A0)
    full = NestedDissectionNormalSolver(A0d)
    print("  full rank, nested dissection (the rows without duplicates)")
    print("      factorization, known pattern %s" % fmt(wall(lambda: NestedDissectionNormalSolver(A0d), sync)))
    P0 = projector.NormalEquationProjector(A0d, full)
    for name, t in operators(P0, n, m0, sync):
        print("      %-2s %s" % (name, fmt(t)))
    for q in DROPPED:
        A, want = with_duplicates(A0, q)
        Ad = dv.DeviceCSR.from_scipy(A)
        m = A.shape[0]
        t0 = time.perf_counter()
        P = SparseDeficientProjector(Ad)
        sync()
        first = 1e3 * (time.perf_counter() - t0)
        assert P.q == q and P.rank == m0, (P.q, P.rank)
        print("  %d duplicated rows appended: dropped %s%s, dependency residual %.1e"
              % (q, P.dropped[:4].tolist(), " ..." if q > 4 else "", P.stats["dependency_residual"]))
        print("      first factorization (host analysis of the new pattern included) %9.3f ms" % first)
        print("      pivot-skipping factorization alone, known pattern %s"
              % fmt(wall(lambda: PivotSkippingNestedSolver(Ad), sync)))
        print("      projector (factorization, %d solves, Woodbury, residual) %s"
              % (q, fmt(wall(lambda: SparseDeficientProjector(Ad), sync))))
        for name, t in operators(P, n, m, sync):
            print("      %-2s %s" % (name, fmt(t)))
        if N == 48:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                svd = lambda: projector.SVDProjector(Ad, 1e-12, 3, 1e-15)
                print("      host exit (SVDProjector): factorization %s" % fmt(wall(svd, sync, reps=3)))
                for name, t in operators(svd(), n, m, sync):
                    print("      host exit %-2s %s" % (name, fmt(t)))


def untouched(lib_path):
    """The normal-mode nested factorization and the dense Cholesky with the library at
    ``lib_path`` (None: this tree's)."""
    import ctypes, torch
    import two_level_cases as tc
    from ipsolver import _hip
    if lib_path:
        probe = ctypes.CDLL(lib_path)
        for name in [k for k in _hip._SIGNATURES if not hasattr(probe, k)]:
            del _hip._SIGNATURES[name]              # (entry points younger than that build)
        _hip.LIB_PATH = lib_path
    from ipsolver import device as dv
    from ipsolver.nested import NestedDissectionNormalSolver
    sync = torch.cuda.synchronize
    _hip.load()
    print("library: %s" % (lib_path or _hip.LIB_PATH), flush=True)
    for N in (100, 316):
        Ad = dv.DeviceCSR.from_scipy(tc.grid(N, 0.125))
        NestedDissectionNormalSolver(Ad)
        print("  nested factorization, normal mode, known pattern, N = %3d %s"
              % (N, fmt(wall(lambda: NestedDissectionNormalSolver(Ad), sync, reps=15))))
    st = dv.stream_ptr()
    for M in (2048, 6400):
        gen = torch.Generator(device="cuda")
        gen.manual_seed(M)
        B = torch.randn((M, M + 64), dtype=torch.float64, device="cuda", generator=gen)
        S = B @ B.t() + M * torch.eye(M, dtype=torch.float64, device="cuda")
        G = torch.empty_like(S)
        flag = torch.zeros(2, dtype=torch.int32, device="cuda")
        work = torch.empty(M + 1, dtype=torch.float64, device="cuda")

        def factor():
            G.copy_(S)
            _hip.call("ipx_chol_factor", M, dv._p(G), dv._p(flag), dv._p(work), st)
        print("  ipx_chol_factor (with the copy of the matrix), M = %4d %s"
              % (M, fmt(wall(factor, sync, reps=15))))


if __name__ == "__main__":
    if "--untouched" in sys.argv:
        untouched(sys.argv[sys.argv.index("--lib") + 1] if "--lib" in sys.argv else None)
    else:
        for N in SIZES:
            measure(N)
