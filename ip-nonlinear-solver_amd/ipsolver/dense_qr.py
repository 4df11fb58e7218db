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
from .dense import block_gemv, block_gemvt
from .device import _p, stream_ptr, ctx
from .factored_projector import FactoredProjector

_F64 = torch.float64

PIVOT_RTOL = 2.0 ** -43          # IPX_PIVOT_RTOL (csrc/ipx_common.h)


class HouseholderQR:
    """``B' = Q R`` for a row-major device tensor ``t`` holding ``B`` (m x n, 1 <= m <= n, leading
    dimension ``lda``).  The constructor enqueues ``ipx_qr_factor``; ``form()`` enqueues ``Q'`` and
    ``R^-T`` and frees the reflectors.  Afterwards: ``QT`` (M x N, row j = column j of Q), ``L`` =
    ``R'`` and ``Linv`` = ``R^-T`` (M x M, lower triangular), M / N = m / n rounded up to 64.
    Device memory while factoring: the padded copy of B that becomes the reflectors and ``QT``
    (both M x N doubles) and the two triangles."""

    def __init__(self, t, m, n, lda):
        lib = _hip.load()
        self.m, self.n = m, n
        self.M, self.N = M, N = int(lib.ipx_dense_padded(m)), int(lib.ipx_qr_padded_cols(n))
        dev = ctx().device
        self._W = torch.empty((M, N), dtype=_F64, device=dev)
        self.L = torch.empty((M, M), dtype=_F64, device=dev)
        self._T = torch.empty((M // 64, 64, 64), dtype=_F64, device=dev)
        tau = torch.empty(M, dtype=_F64, device=dev)
        self._info = torch.empty(M + 1, dtype=_F64, device=dev)
        self._ws = torch.empty(int(lib.ipx_qr_ws_doubles(m, n)), dtype=_F64, device=dev)
        _hip.call("ipx_qr_factor", m, n, _p(t), lda, _p(self._W), _p(self.L), _p(self._T), _p(tau),
                  _p(self._info), _p(self._ws), stream_ptr())
        self._pivot_ratio = None

    @property
    def pivot_ratio(self):
        """``min_j |R_jj| / ||row j of B||`` (0 for a zero row): a blocking read on first use."""
        if self._pivot_ratio is None:
            self._pivot_ratio = float(self._info[0].item())
        return self._pivot_ratio

    def form(self):
        st = stream_ptr()
        self.QT = torch.empty((self.M, self.N), dtype=_F64, device=self.L.device)
        _hip.call("ipx_qr_form_q", self.m, self.n, _p(self._W), _p(self._T), _p(self.QT),
                  _p(self._ws), st)
        self.Linv = torch.empty_like(self.L)
        _hip.call("ipx_qr_tri_inverse", self.M, _p(self.L), _p(self.Linv), st)
        del self._W, self._T, self._ws                  # the reflectors are not needed again
        return self


class DenseQRProjector(FactoredProjector):
    """Z, LS, Y for a ``DeviceDense`` A (m x n, 1 <= m <= n) from ``A' = Q R``.

    ``pivot_ratio``: ``min_j |R_jj| / ||row j of A||`` (0 for a zero row).  ``stats`` counts
    triangular solves and the refinement steps of ``null_space``; LS and Y take none.
    """

    def __init__(self, A, orth_tol=1e-12, max_refin=3):
        FactoredProjector.__init__(self, A, orth_tol, max_refin)
        m, n = A.shape
        if m < 1 or m > n:
            raise np.linalg.LinAlgError("Singular Jacobian matrix: %d rows, %d columns" % (m, n))
        self._qr = qr = HouseholderQR(A.t, m, n, n)
        self.M, self.N = qr.M, qr.N
        self.pivot_ratio = qr.pivot_ratio
        if not self.pivot_ratio >= PIVOT_RTOL:
            raise np.linalg.LinAlgError(
                "numerically rank deficient: min |R_jj| / ||a_j|| = %.3g" % self.pivot_ratio)
        qr.form()
        self._measure_norm_A()

    # -- what the tests read back
    def Q_host(self):
        """Q (n x m) on the host."""
        return self._qr.QT[:self.m, :self.n].t().cpu().numpy()

    def R_host(self):
        """R (m x m, upper triangular) on the host."""
        return self._qr.L[:self.m, :self.m].t().cpu().numpy()

    def _apply_inv(self, x):
        """R^-1 Q' x  (projections.py:192-193)"""
        self.stats["solves"] += 1
        qr = self._qr
        aux1 = block_gemv(qr.QT, qr.N, self.m, self.n, x)
        return block_gemvt(qr.Linv, qr.M, self.m, self.m, aux1)

    def row_space(self, x):                                         # :224-231
        self.stats["solves"] += 1
        qr = self._qr
        aux2 = block_gemv(qr.Linv, qr.M, self.m, self.m, x)         # R^-T x
        return block_gemvt(qr.QT, qr.N, self.m, self.n, aux2)       # Q aux2
