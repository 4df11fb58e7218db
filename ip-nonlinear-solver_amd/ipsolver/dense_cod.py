"""Projections for a RANK-DEFICIENT dense Jacobian on the device (opt-in:
``rank_deficient = "pivoted-qr"``, solver_options.py).  Kernels: csrc/denseqrp.hip and the
block kernels of csrc/denseqr.hip.

Without the option a dense Jacobian that loses a pivot (Gram + Cholesky, dense.py) or fails the
Householder QR's pivot ratio (dense_qr.py) leaves the device: ``SVDProjector`` copies it to the
host and runs LAPACK's SVD there.  ``DenseCODProjector`` keeps it on the device with a complete
orthogonal decomposition from two QR factorizations:

  1. ``A' P = Q1 [R11 R12]`` by a column-pivoted Householder QR of ``A'`` (``ipx_qrp_factor``:
     the reference's own dense method, projections.py:175-233, is a pivoted QR);
  2. the rank ``r``: the number of leading ``j`` with ``|R_jj| > 2^-43 |R_00|``, stopping at the
     first failure -- the project's 43-bit convention (``IPX_PIVOT_RTOL``), RELATIVE where the
     reference's SVD exit is absolute (``s > tol = 1e-15``): an absolute rule keeps or drops the
     spurious singular values of a redundant row, a few eps ``||A||``, depending on the scale of
     ``A`` (DESIGN.md 4o records the reference stalling for that reason);
  3. ``T = [R11 R12]`` (``r x m``) is factored as ``T' = Q2 R2`` by the unpivoted
     ``ipx_qr_factor`` (``T`` row-major with ``r <= m`` is exactly its input form);
  4. ``A' = Q1 R2' Q2' P'``, and with it
        LS x = pinv(A') x = P Q2 R2^-T Q1' x     (the minimum-norm solution, as the SVD's)
        Y b  = pinv(A) b  = Q1 R2^-1 Q2' P' b
        Z x  = x - A' LS x  with the reference's refinement loop (projections.py:248-270).
``P`` is folded into the columns of ``Q2'`` once, ``R2^-1`` is explicit: every operator is two
``ipx_dense_gemv`` / ``ipx_dense_gemvt`` products around one triangular product.

One blocking read per factorization (the rank).  The fused CG loop does not take this projector
(``cg_fused.supports`` is False for it, as for ``SVDProjector``).  A matrix is treated as a
general dense matrix: an ``AugmentedDense``'s structure is not used.  ``1 <= m <= n`` only.
"""
import numpy as np
import torch

from . import _hip
from .dense import block_gemv, block_gemvt
from .dense_qr import HouseholderQR
from .device import DVec, _p, stream_ptr, ctx
from .factored_projector import FactoredProjector

_F64 = torch.float64


class DenseCODProjector(FactoredProjector):
    """Z, LS, Y for a ``DeviceDense`` A (m x n, 1 <= m <= n) of any rank.

    ``rank``; ``pivot_gap``: ``(|R_{r-1,r-1}|, |R_rr|) / |R_00|``, the last kept and the first
    dropped pivot (0 where there is none; the dropped one as the pivot search measured it: the
    remaining column norm); ``stats`` counts solves and the refinement steps of ``null_space``.
    """

    def __init__(self, A, orth_tol=1e-12, max_refin=3):
        lib = _hip.load()
        m, n = A.shape
        if m < 1 or m > n:
            raise np.linalg.LinAlgError("Singular Jacobian matrix: %d rows, %d columns" % (m, n))
        FactoredProjector.__init__(self, A, orth_tol, max_refin)
        M, N = int(lib.ipx_dense_padded(m)), int(lib.ipx_qr_padded_cols(n))
        self.M, self.N = M, N
        dev = ctx().device
        st = stream_ptr()
        W = torch.empty((M, N), dtype=_F64, device=dev)
        self._dw = torch.empty(int(lib.ipx_qrp_info_doubles(m)), dtype=_F64, device=dev)
        self._iw = torch.empty(int(lib.ipx_qrp_info_ints(m)), dtype=torch.int32, device=dev)
        ws = torch.empty(int(lib.ipx_qrp_ws_doubles(m, n)), dtype=_F64, device=dev)
        _hip.call("ipx_qrp_factor", m, n, _p(A.t), n, _p(W), _p(self._dw), _p(self._iw), _p(ws), st)
        done, r = self._iw[2 * M:2 * M + 2].tolist()          # (the one blocking read)
        self.rank = r = int(r)
        assert 0 <= r <= m and (done != 0) == (r < m), (done, r, m)
        self._measure_norm_A()
        del ws
        if r == 0:
            return
        Mr = int(lib.ipx_dense_padded(r))
        self.Mr = Mr
        # Q1' (row j = column j of Q1) from the first r reflectors, in pivot order
        Vp = torch.empty((Mr, N), dtype=_F64, device=dev)
        taup = torch.empty(Mr, dtype=_F64, device=dev)
        _hip.call("ipx_qrp_reflectors", m, n, r, _p(W), _p(self._dw), _p(self._iw), _p(Vp),
                  _p(taup), st)
        T1 = torch.empty((Mr // 64, 64, 64), dtype=_F64, device=dev)
        ws = torch.empty(int(lib.ipx_qr_ws_doubles(r, n)), dtype=_F64, device=dev)
        _hip.call("ipx_qr_wy", r, n, _p(Vp), _p(taup), _p(T1), _p(ws), st)
        Q1T = torch.empty((Mr, N), dtype=_F64, device=dev)
        _hip.call("ipx_qr_form_q", r, n, _p(Vp), _p(T1), _p(Q1T), _p(ws), st)
        # T = [R11 R12] (r x m), then T' = Q2 R2
        R = torch.empty((r, m), dtype=_F64, device=dev)
        _hip.call("ipx_qrp_write_t", m, n, r, _p(W), _p(self._dw), _p(self._iw), _p(R), m, st)
        del W, Vp, T1, ws
        qr2 = HouseholderQR(R, r, m, m).form()          # (its pivot ratio is never read)
        self.N2 = N2 = qr2.N
        # Q2' P': the permutation folded into the columns, once
        Q2TP = torch.zeros((Mr, N2), dtype=_F64, device=dev)
        _hip.call("ipx_qrp_fold_columns", r, m, N2, _p(qr2.QT), _p(self._iw), _p(Q2TP), st)
        self._R, self._Q1T, self._Q2TP, self._L2inv = R, Q1T, Q2TP, qr2.Linv    # (R2^-T)

    # -- what the tests read back
    def perm_host(self):
        """perm[j]: the row of A that is pivot j (the rows beyond the rank in increasing order)."""
        return self._iw[:self.m].cpu().numpy().astype(np.int64)

    def Q1_host(self):
        """Q1 (n x r) on the host."""
        if self.rank == 0:
            return np.zeros((self.n, 0))
        return self._Q1T[:self.rank, :self.n].t().cpu().numpy()

    def R_host(self):
        """[R11 R12] (r x m, columns in pivot order) on the host."""
        if self.rank == 0:
            return np.zeros((0, self.m))
        return self._R.cpu().numpy()

    @property
    def pivot_gap(self):
        r, M = self.rank, self.M
        if r == 0:
            return (0.0, 0.0)
        dw = self._dw.cpu().numpy()
        diag, norms = np.abs(dw[M:M + r]), dw[3 * M:3 * M + r + 1]
        return (float(diag[r - 1] / diag[0]), float(norms[r] / diag[0]) if r < self.m else 0.0)

    def _apply_inv(self, x):
        """pinv(A') x = P Q2 R2^-T Q1' x"""
        self.stats["solves"] += 1
        r = self.rank
        if r == 0:
            return DVec.zeros(self.m)
        aux1 = block_gemv(self._Q1T, self.N, r, self.n, x)
        aux2 = block_gemv(self._L2inv, self.Mr, r, r, aux1)
        return block_gemvt(self._Q2TP, self.N2, r, self.m, aux2)

    def row_space(self, x):                                         # :281-286
        """pinv(A) b = Q1 R2^-1 Q2' P' b"""
        r = self.rank
        if r == 0:
            return DVec.zeros(self.n)
        aux1 = block_gemv(self._Q2TP, self.N2, r, self.m, x)
        aux2 = block_gemvt(self._L2inv, self.Mr, r, r, aux1)
        return block_gemvt(self._Q1T, self.N, r, self.n, aux2)
