"""Seeded inputs of the projected GLTR tests, shared by the host and the GPU tests."""
import numpy as np

SEEDS = (0, 1, 2, 3)
EDGE_K = (1, 2, 63, 64, 65, 255, 256)


def tridiagonals():
    """The 600 seeded tridiagonal trust-region problems of the issue, then one per edge size:
    a list of (diag, off, g0, R)."""
    rng = np.random.default_rng(20260521)
    out = []

    def one(k):
        scale = (1.0, 10.0, 0.1)[rng.integers(3)]
        shift = (0.0, 3.0, -3.0)[rng.integers(3)]
        oscale = (1.0, 0.1)[rng.integers(2)]
        diag = rng.standard_normal(k) * scale + shift
        off = np.abs(rng.standard_normal(max(k - 1, 0))) * oscale + 0.01
        g0 = abs(rng.standard_normal()) + 0.1
        R = 10.0 ** rng.uniform(-3, 2)
        return diag, off, float(g0), float(R)

    for _ in range(600):
        out.append(one(int(rng.integers(1, 257))))
    for k in EDGE_K:
        out.append(one(k))
    return out


# case -> (n, m, eigenvalue range of H, radius, scale of b)
CASES = {
    "A": (40, 8, (-1.0, 4.0), 2.0, 0.0),
    "A'": (40, 8, (-1.0, 4.0), 2.0, 0.1),
    "B": (40, 8, (-4.0, 1.0), 2.0, 0.0),
    "C": (64, 16, (0.5, 4.0), 0.5, 0.0),
    "D": (64, 16, (0.5, 4.0), 50.0, 0.0),
    "E": (200, 40, (-1.0, 4.0), 3.0, 0.0),
}
ON_BOUNDARY = ("A", "A'", "B", "C", "E")
GAINS = ("A", "A'", "B", "E")


def problem(case, seed):
    """(H, c, A, b, radius): b is None where the case has b = 0."""
    n, m, (lo, hi), radius, bscale = CASES[case]
    rng = np.random.default_rng(1000 * seed + sorted(CASES).index(case))
    A = rng.standard_normal((m, n))
    Qm, _ = np.linalg.qr(rng.standard_normal((n, n)))
    H = (Qm * np.linspace(lo, hi, n)) @ Qm.T
    H = 0.5 * (H + H.T)
    c = rng.standard_normal(n)
    b = bscale * rng.standard_normal(m) if bscale else None
    return H, c, A, b, radius


def _rosenbrock_on_planes():
    """The Rosenbrock function of tests/problems.py in ten variables on two hyperplanes through
    its minimiser: equality constraints only, and at the start the Hessian of the Lagrangian
    (the objective's: the constraints are linear) is indefinite."""
    import problems

    class RosenbrockOnPlanes(problems.Rosenbrock):
        def __init__(self):
            problems.Rosenbrock.__init__(self, 10)
            self.name = "rosenbrock10_planes"
            rng = np.random.default_rng(5)
            self.A = rng.integers(-2, 3, (2, 10)).astype(float)
            self.rhs = self.A @ np.ones(10)

        def constraints(self, ns):
            return ns.LinearConstraint(self.A, ("equals", self.rhs))

    return RosenbrockOnPlanes()


def e2e_problems():
    return [_rosenbrock_on_planes()]


def banded_problem():
    """n = 600, m = 60: the banded instance's Jacobian with an indefinite tridiagonal Hessian."""
    import scipy.sparse as sp
    from banded_setup import BandedInstance
    inst = BandedInstance(600, 60)
    n = 600
    rng = np.random.default_rng(11)
    d = np.linspace(-1.0, 3.0, n)[rng.permutation(n)]
    e = 0.3 * rng.standard_normal(n - 1)
    H = sp.diags([e, d, e], [-1, 0, 1], format="csr")
    c = rng.standard_normal(n)
    return H, c, sp.csr_matrix(inst.A), None, 3.0
