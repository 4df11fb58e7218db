"""Householder QR projections for a dense Jacobian on the device (opt-in:
``dense_factorization = "householder-qr"``, solver_options.py).  Kernels: csrc/denseqr.hip.

The reference factors a dense Jacobian by QR of ``A'`` (``qr_factorization_projections``,
projections.py:175-233) and its three operators lose ``cond(A) eps``.  The default here, Gram +
Cholesky (dense.py), loses ``cond(A)^2 eps`` and reports a full-rank Jacobian as singular from
``cond(A)`` of about 1e7.  ``DenseQRProjector`` is the reference's method: ``A' = Q R`` by a
blocked Householder QR on the device, ``Q`` formed explicitly (as ``Q'``, one row per column of
``Q``), ``R^-1`` kept explicitly, and the reference's operators statement by statement
(projections.py:190-231).

Two deviations from the reference, both in how a rank-deficient matrix is recognised:
  * the QR is unpivoted (the reference's is column-pivoted);
  * the test is relative, ``min_j |R_jj| / ||row j of A|| < 2^-43`` -- the project's 43-bit
    convention (``IPX_PIVOT_RTOL``) applied to ``R`` instead of to ``R'R`` -- where the
    reference's is absolute (``||R[-1, :]||_inf < tol``).
A matrix that fails the test leaves by ``np.linalg.LinAlgError``; ``projector._projections``
then warns and takes the SVD exit exactly as for the Cholesky path -- or, under the option
``rank_deficient = "pivoted-qr"``, the device exit of dense_cod.py (``DenseCODProjector``), whose
QR IS column-pivoted and reveals the rank.

The fused CG loop (cg_fused) does not take this projector (``cg_fused.supports`` is False for
anything but a ``NormalEquationProjector``): the CG runs the generic loop, ``qp.projected_cg``.
A matrix is treated as a general dense matrix: an ``AugmentedDense``'s structure is not used.
Norms are plain sums of squares: entries beyond about 1e+-150 are out of scope.
"""
import numpy as np
import torch

from . import _hip
from . import device as dv
from .device import DVec, _p, stream_ptr, ctx

_F64 = torch.float64

PIVOT_RTOL = 2.0 ** -43


class DenseQRProjector:
    """Z, LS, Y for a ``DeviceDense`` A (m x n, 1 <= m <= n) from ``A' = Q R``.

    ``pivot_ratio``: ``min_j |R_jj| / ||row j of A||`` (0 for a zero row).  ``stats`` counts
    triangular solves and the refinement steps of ``null_space``; LS and Y take none.
    Device memory while factoring: the padded copy of A that becomes the reflectors, ``Q'``
    (both ``M x N`` doubles, M / N = m / n rounded up to 64) and two ``M x M`` triangles; the
    reflectors are freed once ``Q'`` is formed.
    """

    def __init__(self, A, orth_tol=1e-12, max_refin=3):
        lib = _hip.load()
        m, n = A.shape
        self.A = A
        self.m, self.n = m, n
        self.orth_tol, self.max_refin = orth_tol, max_refin
        self.stats = {"solves": 0, "refinements": 0}
        if m < 1 or m > n:
            raise np.linalg.LinAlgError("Singular Jacobian matrix: %d rows, %d columns" % (m, n))
        M, N = int(lib.ipx_dense_padded(m)), int(lib.ipx_qr_padded_cols(n))
        self.M, self.N = M, N
        dev = ctx().device
        st = stream_ptr()
        W = torch.empty((M, N), dtype=_F64, device=dev)
        L = torch.empty((M, M), dtype=_F64, device=dev)
        T = torch.empty((M // 64, 64, 64), dtype=_F64, device=dev)
        tau = torch.empty(M, dtype=_F64, device=dev)
        info = torch.empty(M + 1, dtype=_F64, device=dev)
        ws = torch.empty(int(lib.ipx_qr_ws_doubles(m, n)), dtype=_F64, device=dev)
        _hip.call("ipx_qr_factor", m, n, _p(A.t), n, _p(W), _p(L), _p(T), _p(tau), _p(info),
                  _p(ws), st)
        self.pivot_ratio = float(info[0].item())
        self._L = L                                     # R' (lower triangular, padded)
        if not self.pivot_ratio >= PIVOT_RTOL:
            raise np.linalg.LinAlgError(
                "numerically rank deficient: min |R_jj| / ||a_j|| = %.3g" % self.pivot_ratio)
        QT = torch.empty((M, N), dtype=_F64, device=dev)
        _hip.call("ipx_qr_form_q", m, n, _p(W), _p(T), _p(QT), _p(ws), st)
        Linv = torch.empty((M, M), dtype=_F64, device=dev)
        _hip.call("ipx_qr_tri_inverse", M, _p(L), _p(Linv), st)
        del W, T, ws                                    # the reflectors are not needed again
        self._QT, self._Linv = QT, Linv
        self.norm_A = A.frobenius_norm()

    # -- what the tests read back
    def Q_host(self):
        """Q (n x m) on the host."""
        return self._QT[:self.m, :self.n].t().cpu().numpy()

    def R_host(self):
        """R (m x m, upper triangular) on the host."""
        return self._L[:self.m, :self.m].t().cpu().numpy()

    # -- device products
    def _gemv(self, B, ldb, rows, cols, x):
        """B[:rows, :cols] x"""
        out = DVec(dv._empty(rows))
        _hip.call("ipx_dense_gemv", rows, cols, _p(B), ldb, _p(x.t), 1.0, None, 0.0, None,
                  _p(out.t), None, None, stream_ptr())
        return out

    def _gemvt(self, B, ldb, rows, cols, x):
        """B[:rows, :cols]' x"""
        out = DVec(dv._empty(cols))
        _hip.call("ipx_dense_gemvt", rows, cols, _p(B), ldb, _p(x.t), _p(out.t), stream_ptr())
        return out

    def _solve(self, x):
        """R^-1 Q' x  (projections.py:192-193)"""
        self.stats["solves"] += 1
        aux1 = self._gemv(self._QT, self.N, self.m, self.n, x)
        return self._gemvt(self._Linv, self.M, self.m, self.m, aux1)

    def _orth(self, z):
        norm_z = dv.norm(z)
        if norm_z == 0 or self.norm_A == 0:
            return 0.0
        return dv.norm(self.A.dot(z)) / (self.norm_A * norm_z)

    def null_space(self, x):                                        # :190-212
        z = self.A.rmatvec_sub(self._solve(x), x)
        k = 0
        while self._orth(z) > self.orth_tol:
            if k >= self.max_refin:
                break
            z = self.A.rmatvec_sub(self._solve(z), z)
            k += 1
            self.stats["refinements"] += 1
        return z

    def least_squares(self, x):                                     # :215-221
        return self._solve(x)

    def row_space(self, x):                                         # :224-231
        self.stats["solves"] += 1
        aux2 = self._gemv(self._Linv, self.M, self.m, self.m, x)    # R^-T x
        return self._gemvt(self._QT, self.N, self.m, self.n, aux2)  # Q aux2

    def operators(self):
        from .projector import _Op
        ops = (_Op((self.n, self.n), self.null_space),
               _Op((self.m, self.n), self.least_squares),
               _Op((self.n, self.m), self.row_space))
        for op in ops:
            op.projector = self
        return ops
