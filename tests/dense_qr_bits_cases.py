"""What the dense QR projectors (ipsolver/dense_qr.py, ipsolver/dense_cod.py; csrc/denseqr.hip,
csrc/denseqrp.hip) compute, case by case, as arrays to be compared BIT FOR BIT with
tests/golden/dense_qr_bits.npz (tests/test_gpu_dense_qr_bits.py; written by
``tests/golden/make_golden.py --dense-qr-bits`` on the GPU).

Every case is a function without arguments that returns ``{key: numpy array}``; an array of more
than 512 entries is stored as its digest (pcr_family_cases.digest).  Inputs are the seeded
builders of the tolerance tests: test_gpu_dense_qr's Gaussian / ``graded`` matrices and
rank_deficient_cases.build.  ``counts`` holds the deltas of the library's launch and blocking-read
counters: (launches, reads) of the construction, then of the three operator calls together.
``SVDProjector`` factors with the host's LAPACK: its bits are not recorded.
"""
import warnings

import numpy as np

from pcr_family_cases import digest

# (m, n, kind): a single row; one panel exactly; panel + 1; two panels + 2 with a ragged n and
# two chunks of 512 columns; nine panels, the last with first chunk c0 = 1; ill-conditioned input
QR_SHAPES = [(1, 5, "normal"), (64, 64, "normal"), (65, 300, "normal"), (130, 700, "normal"),
             (520, 2100, "normal"), (130, 700, "graded")]

# rank 0 (returns early) and low rank; the usual shapes; (520, 2100): the only pivoted case whose
# steps reach the first chunk c0 = j / 512 >= 1
COD_CASES = [("zeros-all-3x5", ("zeros-all", 3, 5)),
             ("lowrank-3x5", ("lowrank", 3, 5)),
             ("duplicate-64x64", ("duplicate", 64, 64)),
             ("combination-65x300", ("combination", 65, 300)),
             ("zero-130x700", ("zero", 130, 700)),
             ("lowrank-130x700", ("lowrank", 130, 700)),
             ("graded-130x700-k5-1e+06", ("graded", 130, 700, 5, 1e6)),
             ("duplicate-520x2100", ("duplicate", 520, 2100))]


class counters:
    """(launches, blocking reads) of the library over a block."""

    def __enter__(self):
        from ipsolver import _hip
        self.lib = _hip.load()
        self.start = (int(self.lib.ipx_launch_count()), int(self.lib.ipx_read_count()))
        return self

    def __exit__(self, *exc):
        self.delta = (int(self.lib.ipx_launch_count()) - self.start[0],
                      int(self.lib.ipx_read_count()) - self.start[1])


def _host(v):
    return digest(v.to_host())


def operators(P, rng, m, n):
    """Z x, LS x, Y b of a projector (or of its operator triple) on ``default_rng`` vectors, and
    the counter deltas of the three calls."""
    import ipsolver.device as dv
    x = dv.DVec.from_host(rng.standard_normal(n))
    b = dv.DVec.from_host(rng.standard_normal(m))
    Z, LS, Y = P.operators() if hasattr(P, "operators") else P
    with counters() as c:
        z, ls, y = Z.dot(x), LS.dot(x), Y.dot(b)
    return {"Z": _host(z), "LS": _host(ls), "Y": _host(y)}, c.delta


def _stats(P):
    return np.array([P.stats[k] for k in sorted(P.stats)], dtype=np.int64)


def qr_matrix(m, n, kind):
    import test_gpu_dense_qr as t1
    rng = np.random.default_rng(1000 * m + n)
    A = rng.standard_normal((m, n)) if kind == "normal" else t1.graded(rng, m, n, 1e10)
    return A, rng


def householder(m, n, kind):
    from ipsolver.dense import DeviceDense
    from ipsolver.dense_qr import DenseQRProjector
    A, rng = qr_matrix(m, n, kind)
    D = DeviceDense.from_host(A)
    with counters() as made:
        P = DenseQRProjector(D)
    out = {"Q": digest(P.Q_host()), "R": digest(P.R_host()),
           "pivot_ratio": np.array([P.pivot_ratio])}
    ops, called = operators(P, rng, m, n)
    out.update(ops)
    out["stats"] = _stats(P)
    out["counts"] = np.array(made.delta + called, dtype=np.int64)
    return out


def pivoted(args):
    import rank_deficient_cases
    from ipsolver.dense import DeviceDense
    from ipsolver.dense_cod import DenseCODProjector
    A, _ = rank_deficient_cases.build(*args)
    m, n = A.shape
    D = DeviceDense.from_host(A)
    with counters() as made:
        P = DenseCODProjector(D)
    out = {"rank": np.array([P.rank], dtype=np.int64), "perm": digest(P.perm_host()),
           "Q1": digest(P.Q1_host()), "R": digest(P.R_host()),
           "pivot_gap": np.array(P.pivot_gap)}
    ops, called = operators(P, np.random.default_rng(m + n), m, n)
    out.update(ops)
    out["stats"] = _stats(P)
    out["counts"] = np.array(made.delta + called, dtype=np.int64)
    return out


def _solver_name(proj):
    return np.frombuffer(str(proj.last_normal_solver()).encode(), dtype=np.uint8).copy()


def public_householder():
    """``projections(D)`` under ``dense_factorization = "householder-qr"`` on Gaussian (65, 300)."""
    import ipsolver.projector as proj
    from ipsolver.dense import DeviceDense
    A, rng = qr_matrix(65, 300, "normal")
    with proj.dense_factorization("householder-qr"):
        ops = proj.projections(DeviceDense.from_host(A))
        out, _ = operators(ops, rng, 65, 300)
        out["solver"] = _solver_name(proj)
    return out


def public_pivoted():
    """``projections(D)`` under ``rank_deficient = "pivoted-qr"`` on ``duplicate-65x300`` (the
    Cholesky factorization loses a pivot; the exit is the device's)."""
    import rank_deficient_cases
    import ipsolver.projector as proj
    from ipsolver.dense import DeviceDense
    A, _ = rank_deficient_cases.build("duplicate", 65, 300)
    with proj.rank_deficient("pivoted-qr"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ops = proj.projections(DeviceDense.from_host(A))
        out, _ = operators(ops, np.random.default_rng(365), 65, 300)
        out["solver"] = _solver_name(proj)
    return out


CASES = {}
for _m, _n, _kind in QR_SHAPES:
    CASES["qr-%s-%dx%d" % (_kind, _m, _n)] = (lambda a=(_m, _n, _kind): householder(*a))
for _name, _args in COD_CASES:
    CASES["cod-" + _name] = (lambda a=_args: pivoted(a))
CASES["public-householder-qr"] = public_householder
CASES["public-pivoted-qr"] = public_pivoted


def record(log=print):
    """Every case -> {"<case>/<key>": array}."""
    out = {}
    for name, fn in CASES.items():
        got = fn()
        for k, v in got.items():
            out[name + "/" + k] = v
        log("case %s: %d arrays, %d bytes" % (name, len(got), sum(v.nbytes for v in got.values())))
    return out
