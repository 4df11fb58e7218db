"""What the projectors share: the operator object handed to callers and, for the projectors that
hold a factorization of ``A`` itself (SVD, Householder QR, complete orthogonal decomposition), the
reference's refinement loop.  Below projector.py in the import order.
"""
from . import device as dv
from .device import DVec


class _Op:
    """Operator object returned by ``projections`` (duck type of scipy's
    LinearOperator as used by the reference: shape / dot / matvec)."""

    def __init__(self, shape, fn):
        self.shape = shape
        self._fn = fn

    def dot(self, x):
        return self._fn(x if isinstance(x, DVec) else DVec.from_host(x))

    matvec = dot


def operator_triple(P):
    """(Z, LS, Y) of a projector with ``null_space``, ``least_squares``, ``row_space``."""
    ops = (_Op((P.n, P.n), P.null_space),
           _Op((P.m, P.n), P.least_squares),
           _Op((P.n, P.m), P.row_space))
    for op in ops:
        op.projector = P         # lets the fused CG loop recognise its own operators
    return ops


class FactoredProjector:
    """Z, LS, Y from a factorization of ``A``.  A subclass supplies ``_apply_inv(x)`` =
    ``pinv(A') x`` -- which counts itself in ``stats["solves"]`` -- and ``row_space(b)`` =
    ``pinv(A) b``, and sets ``norm_A``; ``stats`` also counts the refinement steps of
    ``null_space``."""

    def __init__(self, A, orth_tol, max_refin):
        self.A = A
        self.m, self.n = A.shape
        self.orth_tol, self.max_refin = orth_tol, max_refin
        self.stats = {"solves": 0, "refinements": 0}

    def _measure_norm_A(self):
        """``||A||_F`` (a blocking read, taken where the subclass's factorization is done)."""
        self.norm_A = self.A.frobenius_norm() if self.m > 0 else 0.0

    def _orth(self, z):
        """``||A z|| / (||A||_F ||z||)`` (projections.py:23-55)"""
        norm_z = dv.norm(z)
        if norm_z == 0 or self.norm_A == 0:
            return 0.0
        return dv.norm(self.A.dot(z)) / (self.norm_A * norm_z)

    def null_space(self, x):                        # projections.py:190-212 / 248-270
        z = self.A.rmatvec_sub(self._apply_inv(x), x)
        k = 0
        while self._orth(z) > self.orth_tol:
            if k >= self.max_refin:
                break
            z = self.A.rmatvec_sub(self._apply_inv(z), z)
            k += 1
            self.stats["refinements"] += 1
        return z

    def least_squares(self, x):                     # :215-221 / 273-278
        return self._apply_inv(x)

    def operators(self):
        return operator_triple(self)
