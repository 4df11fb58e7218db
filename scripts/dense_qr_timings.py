"""The Householder QR projections of a dense Jacobian (ipsolver/dense_qr.py, csrc/denseqr.hip;
``dense_factorization = "householder-qr"``) next to the default, Gram + Cholesky + explicit
inverse (``DenseNormalSolver``), on the same matrices in the same run.  Per (m, n):
  * the factorization (QR: factor + form Q + triangular inverse; default: Gram + Cholesky +
    inverse), milliseconds and kernel launches;
  * milliseconds per Z, LS and Y call of both.
Then the accuracy table of tests/test_gpu_dense_qr.py::test_factorization_against_lapack: the
orthogonality max|Q'Q - I| and the backward error max|A' - QR| / max|A| in units of eps, next to
LAPACK's on the same input.
Times are HIP event timings around work that includes its own blocking reads; medians of REPS
runs after WARM warm-up runs, the smallest and largest beside them; one process.  The output
goes to profiles/dense_qr_timings.txt as well.
    python scripts/dense_qr_timings.py"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ip-nonlinear-solver_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = [(200, 1000), (800, 4000), (2000, 10000)]
WARM, REPS = 2, 7
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def timed(fn, reps=REPS, warm=WARM):
    """(median, min, max) in ms of fn() between two HIP events."""
    import torch
    out = []
    for k in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if k >= warm:
            out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def fmt(t):
    return "%9.3f ms (%.3f .. %.3f)" % t


def main():
    import numpy as np
    import torch
    from ipsolver import _hip, device as dv, projector
    from ipsolver.dense import DeviceDense, DenseNormalSolver
    from ipsolver.dense_qr import DenseQRProjector
    import test_gpu_dense_qr as t1
    lib = _hip.load()
    say("dense QR projections against Gram + Cholesky  (%s)" % torch.cuda.get_device_name(0))
    for m, n in SIZES:
        rng = np.random.default_rng(m)
        A = rng.standard_normal((m, n))
        D = DeviceDense.from_host(A)
        D.T                                            # (the transposed copy both paths use)
        x = dv.DVec.from_host(rng.standard_normal(n))
        b = dv.DVec.from_host(rng.standard_normal(m))
        say("\n== m = %d, n = %d" % (m, n))
        count = {}
        for name, make in (("householder-qr", lambda: DenseQRProjector(D)),
                           ("normal-equations", lambda: DenseNormalSolver(D))):
            make()
            before = lib.ipx_launch_count()
            make()
            count[name] = lib.ipx_launch_count() - before
            say("  factorization  %-17s %s  %5d launches" % (name, fmt(timed(make)), count[name]))
        for name in ("householder-qr", "normal-equations"):
            projector.invalidate(D)
            with projector.dense_factorization(name):
                Z, LS, Y = projector.projections(D)
                for label, op, v in (("Z", Z, x), ("LS", LS, x), ("Y", Y, b)):
                    say("  %-2s per call    %-17s %s" % (label, name, fmt(timed(lambda: op.dot(v)))))
    say("\n== accuracy (units of eps; LAPACK's np.linalg.qr(A.T) on the same input beside it)")
    say("   normal: standard normal entries; graded: U diag(logspace(0, -10, m)) V'")
    eps = np.finfo(float).eps
    for m, n in t1.SHAPES + SIZES[1:]:
        for kind in ("normal", "graded"):
            if kind == "graded" and m == 1:
                continue
            rng = np.random.default_rng(1000 * m + n)
            A = rng.standard_normal((m, n)) if kind == "normal" else t1.graded(rng, m, n, 1e10)
            P = DenseQRProjector(DeviceDense.from_host(A))
            orth, back = t1.identities(A, P.Q_host(), P.R_host())
            ol, bl = t1.identities(A, *np.linalg.qr(A.T))
            say("  (%4d, %5d) %-6s  orthogonality %6.2f (LAPACK %6.2f)   backward %6.2f "
                "(LAPACK %6.2f)" % (m, n, kind, orth / eps, ol / eps, back / eps, bl / eps))
    with open(os.path.join(ROOT, "profiles", "dense_qr_timings.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
