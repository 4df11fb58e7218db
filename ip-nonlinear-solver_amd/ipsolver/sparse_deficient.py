"""Projections for a RANK-DEFICIENT sparse Jacobian on the device (opt-in:
``sparse_rank_deficient = "skip-pivots"``, solver_options.py).  Kernels: the skip mode of
csrc/nested.hip / csrc/dense.hip and the q x q Woodbury kernels of csrc/bordered.hip.

Without the option a sparse Jacobian whose ``A A'`` loses a pivot leaves the device: ``SVDProjector``
copies it to the host as a dense matrix (``m n <= 2^25``) and runs LAPACK's SVD there.  Here it is
factored once more by the nested-dissection Cholesky in skip mode (``PivotSkippingNestedSolver``):
a pivot that vanishes is a row that depends on the rows eliminated before it, and dropping it
leaves the factorization of ``A_S A_S'``, S a maximal independent row set, D the q dropped rows.
``K+ w`` is that solver's solve: ``(A_S A_S')^-1 w_S`` on S, 0 on D.

With ``A_D = W A_S``, ``W = A_D A_S' (A_S A_S')^-1``: ``A = B A_S``, ``B = [I; W]`` in row order,
    pinv(A) = A_S' (A_S A_S')^-1 (I + W'W)^-1 B',    (I + W'W)^-1 = I - W' C^-1 W,  C = I_q + W W'.
``Yw`` (column-major m x q) holds ``W'`` with zero rows at D; column j is ``K+ (A a_dj')``, q solves
at factorization time; ``C = I + Yw' Yw`` by ``ipx_border_gram`` / ``ipx_border_chol``.

    Z x  = x - A' K+ A x                      no correction: what a full-rank projection costs
    LS x = pinv(A') x:   u = K+ A x;  u <- u - Yw C^-1 Yw' u;  out_S = u,  out_D = Yw' u
    Y b  = pinv(A) b:    t_S = b_S + (Yw b_D)_S;  t <- t - Yw C^-1 Yw' t;  out = A' K+ t
                         (and one refinement step on b - A out: ``ROW_SPACE_REFINE``)

the signs as every projector of this package and the oracle have them.  ``rank == m`` (the first
solver's complaint was a false alarm) is legal: the operators are the plain normal-equation ones.
The fused CG loop does not take this projector (as ``SVDProjector``).
"""
import numpy as np
import torch

from . import _hip
from . import device as dv
from .device import DVec, _p, stream_ptr, ctx
from .factored_projector import FactoredProjector
from .nested import PivotSkippingNestedSolver

_F64 = torch.float64


class SparseDeficientProjector(FactoredProjector):
    """Z, LS, Y for a ``DeviceCSR`` A (m >= 1) of any rank, at most ``ipx_border_pmax()`` rows
    dropped (``LinAlgError`` past that; ``NestedDissectionRefused`` past the nested solver's
    limits).

    ``rank``, ``dropped`` (ascending rows, host); ``stats``: solves, refinements, rank, dropped
    (their number) and ``dependency_residual`` = max_j ||a_dj - A_S' w_j||_inf / ||a_dj||_inf
    (0 for a zero row), measured once per factorization and not thresholded."""

    solver_class = PivotSkippingNestedSolver

    def __init__(self, A, orth_tol=1e-12, max_refin=3):
        lib = _hip.load()
        FactoredProjector.__init__(self, A, orth_tol, max_refin)
        m = self.m
        if m < 1:
            raise np.linalg.LinAlgError("Singular Jacobian matrix: no rows")
        self.solver = self.solver_class(A)
        self.dropped = self.solver.dropped
        self.rank, self.q = self.solver.rank, len(self.dropped)
        q, most = self.q, int(lib.ipx_border_pmax())
        if q > most:
            raise np.linalg.LinAlgError(
                "Singular Jacobian matrix: %d dependent rows, the pivot-skipping factorization "
                "corrects for <= %d" % (q, most))
        self._measure_norm_A()
        self.stats.update(rank=self.rank, dropped=q, dependency_residual=0.0)
        if q == 0:
            return
        dev = ctx().device
        G = int(lib.ipx_border_groups(m))
        # one tensor owns everything: [Yw | K | L | info | Gram partials | t partials]
        sizes = (m * q, q * q, q * q, 2, G * q * q, G * q)
        self.ws = torch.zeros(int(sum(sizes)), dtype=_F64, device=dev)
        self.Yw, self.K, self.L, self.info, self._gpart, self._tpart = \
            torch.split(self.ws, list(sizes))
        self._d_rows = torch.from_numpy(np.ascontiguousarray(self.dropped)).to(dev)
        # rows a_dj as columns (n x q, a unit vector through A'), then Yw = K+ (A a_dj')
        E = torch.zeros((q, m), dtype=_F64, device=dev)
        E[torch.arange(q, device=dev), self._d_rows.long()] = 1.0
        rows = [A.T.dot(dv._wrap(E[j])) for j in range(q)]
        for j in range(q):
            yj = self.solver.solve(A.dot(rows[j]))
            self.Yw[j * m:(j + 1) * m].copy_(yj.t)
        _hip.call("ipx_border_gram", m, q, _p(self.Yw), _p(self.Yw), _p(self._gpart), stream_ptr())
        _hip.call("ipx_border_chol", m, q, _p(self._gpart), _p(self.K), _p(self.L), _p(self.info),
                  stream_ptr())
        # a_dj - A_S' w_j = a_dj - A' Yw[:, j] (zero rows at D), against ||a_dj||_inf: one read
        res = torch.stack([A.rmatvec_sub(dv._wrap(self.Yw[j * m:(j + 1) * m]), rows[j]).t
                           for j in range(q)]).abs().amax(dim=1)
        ref = torch.stack([r.t for r in rows]).abs().amax(dim=1)
        res, ref = res.cpu().numpy(), ref.cpu().numpy()
        ratio = np.divide(res, ref, out=np.zeros(q), where=ref > 0)
        self.stats["dependency_residual"] = float(ratio.max())

    def _kplus(self, w):
        self.stats["solves"] += 1
        return self.solver.solve(w)

    def _woodbury(self, u):
        """u <- u - Yw C^-1 Yw' u, in place"""
        m, q = self.m, self.q
        _hip.call("ipx_border_tdot", m, q, _p(self.Yw), _p(u.t), _p(self._tpart), stream_ptr())
        _hip.call("ipx_border_apply", m, q, _p(self.Yw), _p(self.L), _p(self._tpart), _p(u.t),
                  _p(u.t), stream_ptr())
        return u

    def _apply_inv(self, x):
        """pinv(A') x"""
        u = self._kplus(self.A.dot(x))
        if self.q == 0:
            return u
        m, q = self.m, self.q
        u = self._woodbury(u)
        _hip.call("ipx_border_tdot", m, q, _p(self.Yw), _p(u.t), _p(self._tpart), stream_ptr())
        out = dv._empty(m)
        _hip.call("ipx_nd_dropped_fill", m, q, _p(self._tpart), _p(self._d_rows),
                  _p(self.solver.mark), _p(u.t), _p(out), stream_ptr())
        return DVec(out)

    def null_space(self, x):
        """x - A' K+ A x: K+ uncorrected, the base class's refinement loop around it"""
        z = self.A.rmatvec_sub(self._kplus(self.A.dot(x)), x)
        k = 0
        while self._orth(z) > self.orth_tol:
            if k >= self.max_refin:
                break
            z = self.A.rmatvec_sub(self._kplus(self.A.dot(z)), z)
            k += 1
            self.stats["refinements"] += 1
        return z

    def _row_space0(self, b):
        if self.q == 0:
            return self.A.T.dot(self._kplus(b))
        m, q = self.m, self.q
        t = dv._empty(m)
        _hip.call("ipx_nd_dropped_fold", m, q, _p(self.Yw), _p(self._d_rows),
                  _p(self.solver.mark), _p(b.t), _p(t), stream_ptr())
        return self.A.T.dot(self._kplus(self._woodbury(DVec(t))))

    # The normal equations leave A y - b at cond(A_S)^2 eps ||b|| -- the residual of the solve
    # with A_S A_S' -- where the outer loops' normal step wants A y = b to rounding (the
    # reference's own exit, an SVD, gives cond eps).  One step on the residual, a second
    # application per call (once per outer iteration, never inside the CG loop), removes the
    # square: measured on the pure incidence matrix of the 12 x 12 grid, cond(A_S) = 40.
    ROW_SPACE_REFINE = 1

    def row_space(self, b):
        """pinv(A) b"""
        y = self._row_space0(b)
        for _ in range(self.ROW_SPACE_REFINE):
            y = y + self._row_space0(self.A.spmv(y, alpha=-1.0, beta=1.0, yin=b))
        return y
