"""The device exit for rank-deficient dense Jacobians (ipsolver/dense_cod.py,
csrc/denseqrp.hip; ``rank_deficient = "pivoted-qr"``) next to the host exit it replaces
(``SVDProjector``: copy to the host, ``scipy.linalg.svd``, upload of the factors), on the same
matrices in the same run.  Per (m, n) and rank (m - 1: one duplicated row; m / 2: a product of
two Gaussian factors):
  * the factorization, milliseconds (device: the pivoted QR through Q1', Q2'P' and R2^-1, with
    its one blocking read) and kernel launches;
  * milliseconds per Z, LS and Y call of both.
Times are HIP event timings around work that includes its own blocking reads (and, for the host
exit, the host's LAPACK call); medians of the runs after the warm-up runs, the smallest and
largest beside them; one process.  The output goes to profiles/dense_cod_timings.txt as well.
    python scripts/dense_cod_timings.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ip-nonlinear-solver_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from dense_qr_timings import timed, fmt, SIZES  # noqa: E402

LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def main():
    import numpy as np
    import torch
    from ipsolver import _hip, device as dv
    from ipsolver.dense import DeviceDense
    from ipsolver.dense_cod import DenseCODProjector
    from ipsolver.projector import SVDProjector
    lib = _hip.load()
    say("rank-deficient dense Jacobians: pivoted QR on the device against the host SVD  (%s)"
        % torch.cuda.get_device_name(0))
    for m, n in SIZES:
        for rank in (m - 1, m // 2):
            rng = np.random.default_rng(m + rank)
            if rank == m - 1:
                A = rng.standard_normal((m, n))
                A[m - 3] = A[5]
            else:
                A = rng.standard_normal((m, rank)) @ rng.standard_normal((rank, n)) / np.sqrt(rank)
            A *= 2.0 ** -10
            D = DeviceDense.from_host(A)
            D.T                                        # (the transposed copy both paths use)
            x = dv.DVec.from_host(rng.standard_normal(n))
            b = dv.DVec.from_host(rng.standard_normal(m))
            say("\n== m = %d, n = %d, rank %d" % (m, n, rank))
            made = {}
            for name, make, reps in (("pivoted-qr", lambda: DenseCODProjector(D), 5),
                                     ("host-svd", lambda: SVDProjector(D, 1e-12, 3, 1e-15), 3)):
                before = lib.ipx_launch_count()
                made[name] = make()
                launches = lib.ipx_launch_count() - before
                assert made[name].rank == rank, (name, made[name].rank)
                say("  factorization  %-11s %s  %5d launches"
                    % (name, fmt(timed(make, reps=reps, warm=1)), launches))
            say("  pivot gap %.3g | %.3g" % made["pivoted-qr"].pivot_gap)
            for name, P in made.items():
                for label, op, v in (("Z", P.null_space, x), ("LS", P.least_squares, x),
                                     ("Y", P.row_space, b)):
                    say("  %-2s per call    %-11s %s" % (label, name, fmt(timed(lambda: op(v)))))
    with open(os.path.join(ROOT, "profiles", "dense_cod_timings.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
