"""Dense Jacobian path (BASELINE config 2): device matrix + Gram/Cholesky
normal-equation solver.  Kernels: csrc/dense.hip.

The reference factors dense Jacobians with LAPACK pivoted QR
(projections.py:175-233).  Here ``G = A A'`` is formed with fp64 MFMA,
factored by a blocked Cholesky, and ``G^-1`` is kept explicitly so that each
``(AA')^-1`` application inside the CG loop is one dense matvec (6 us instead of two
latency-bound triangular sweeps of 63 dependent tile steps each).  Applying the explicit
inverse is as accurate as two triangular solves with the factor -- both are limited by
the normal equations, cond(A)^2 eps: measured 3.0e-5 vs 1.1e-5 at cond(A) = 1e6,
scripts/exp_ill_conditioned_dense.py and tests/test_gpu_qp.py::test_dense_ill_conditioned --
and what the normal equations lose against the reference's QR is recovered by refinement
steps (``refine_steps``, enabled from the measured pivot loss).  The
operators are the same (QR vs Gram-Cholesky iterates
agree to 8e-16 on well-conditioned problems); a rank-deficient Jacobian is
reported through the pivot flag.
"""
import ctypes
import warnings

import numpy as np
import torch

from . import _hip
from . import device as dv
from .device import DVec, _p, stream_ptr, ctx

_F64 = torch.float64


class DeviceDense:
    """Row-major dense fp64 matrix in HBM with ``dot`` / ``T.dot`` (the
    transpose is materialised once: both products are row-streaming matvecs)."""

    def __init__(self, t):
        assert t.dtype == _F64 and t.dim() == 2 and t.is_cuda
        self.t = t if t.is_contiguous() else t.contiguous()
        self.shape = (int(t.shape[0]), int(t.shape[1]))
        self._T = None

    @staticmethod
    def from_host(a):
        dv._require_gpu()
        a = np.ascontiguousarray(np.atleast_2d(np.asarray(a, dtype=np.float64)))
        with warnings.catch_warnings():        # (a read-only host array is only read here)
            warnings.simplefilter("ignore", UserWarning)
            return DeviceDense(torch.from_numpy(a).to(ctx().device))

    def to_host(self):
        return self.t.cpu().numpy()

    @property
    def T(self):
        if self._T is None:
            self._T = DeviceDense(self.t.t().contiguous())     # layout copy, no arithmetic
            self._T._T = self
        return self._T

    def gemv(self, x, alpha=1.0, diag=None, beta=0.0, yin=None, reduce=False, slot=0):
        m, n = self.shape
        assert len(x) == n, (len(x), n)
        out = DVec(dv._empty(m))
        c = ctx()
        _hip.call("ipx_dense_gemv", m, n, _p(self.t), n, _p(x.t), float(alpha),
                  _p(diag.t) if diag is not None else None, float(beta),
                  _p(yin.t) if yin is not None else None, _p(out.t),
                  ctypes.c_void_p(c.out.data_ptr() + 16 * slot) if reduce else None,
                  _p(c.ws), stream_ptr())
        return out

    spmv = gemv

    def dot(self, x):
        return self.gemv(x if isinstance(x, DVec) else DVec.from_host(x))

    matvec = dot

    def matvec_sumsq(self, x, slot=0):
        out = self.gemv(x, reduce=True, slot=slot)
        return out, dv.read_slots(2 * slot + 1)[2 * slot]

    def rmatvec_sub(self, v, x, reduce=False, slot=0):
        return self.T.gemv(v, alpha=-1.0, beta=1.0, yin=x, reduce=reduce, slot=slot)

    def frobenius_norm(self):
        return dv.norm(DVec(self.t.reshape(-1)))


def block_gemv(B, ldb, rows, cols, x):
    """``B[:rows, :cols] x`` for the leading block of a row-major device tensor ``B`` (leading
    dimension ``ldb``: the padded factors of dense_qr.py / dense_cod.py)."""
    out = DVec(dv._empty(rows))
    _hip.call("ipx_dense_gemv", rows, cols, _p(B), ldb, _p(x.t), 1.0, None, 0.0, None,
              _p(out.t), None, None, stream_ptr())
    return out


def block_gemvt(B, ldb, rows, cols, x):
    """``B[:rows, :cols]' x`` without a transposed copy."""
    out = DVec(dv._empty(cols))
    _hip.call("ipx_dense_gemvt", rows, cols, _p(B), ldb, _p(x.t), _p(out.t), stream_ptr())
    return out


class AugmentedDense(DeviceDense):
    """The barrier's augmented Jacobian ``A = [[J_eq, 0], [J_ineq, diag(s)]]`` assembled from a
    device-mode dense canonical Jacobian (``device_mode.DenseStack``).  Its normal matrix is
    structured, ``A A' = J J' + diag(0_{m_eq}, s*s)``: ``DenseNormalSolver`` forms the Gram of
    the first ``n_vars`` columns only and shifts its diagonal (the slacks read off A's diagonal
    block), and -- the canonical Jacobian being constant (``stack.constant``: linear and box
    constraints only) -- keeps ``J J'`` for the whole solve in ``stack.gram0``."""

    def __init__(self, t, n_vars, m_eq, stack):
        DeviceDense.__init__(self, t)
        self.n_vars, self.m_eq, self.stack = int(n_vars), int(m_eq), stack


def augment(J_eq, J_ineq, s, n_vars, n_eq, n_ineq, stack=None):
    """``[[J_eq, 0], [J_ineq, diag(s)]]`` (tr_interior_point.py:141-194) and its transpose in one
    launch (csrc/densejac.hip) from row-major device blocks ``J_eq`` / ``J_ineq`` (tensors,
    leading dimension ``n_vars``).  The transpose becomes the result's cached ``.T``.  With
    ``stack`` (device-callback mode) the result is an ``AugmentedDense``."""
    dev = ctx().device
    m, N = n_eq + n_ineq, n_vars + n_ineq
    assert J_eq.shape == (n_eq, n_vars) and J_ineq.shape == (n_ineq, n_vars), \
        (J_eq.shape, J_ineq.shape, n_eq, n_ineq, n_vars)
    assert len(s) == n_ineq and J_eq.is_contiguous() and J_ineq.is_contiguous()
    A = torch.empty((m, N), dtype=_F64, device=dev)
    At = torch.empty((N, m), dtype=_F64, device=dev)
    _hip.call("ipx_dense_augment", n_eq, n_ineq, n_vars, _p(J_eq) if n_eq else None, n_vars,
              _p(J_ineq) if n_ineq else None, n_vars, _p(s.t), _p(A), _p(At), stream_ptr())
    out = DeviceDense(A) if stack is None else AugmentedDense(A, n_vars, n_eq, stack)
    out._T = DeviceDense(At)
    out._T._T = out
    return out


def transpose_into(D):
    """Give a DeviceDense its cached ``.T`` through the augment kernel (no torch transpose)."""
    m, n = D.shape
    if D._T is None and m and n:
        At = torch.empty((n, m), dtype=_F64, device=ctx().device)
        _hip.call("ipx_dense_augment", m, 0, n, _p(D.t), n, None, n, None, None, _p(At),
                  stream_ptr())
        D._T = DeviceDense(At)
        D._T._T = D
    return D


class DenseNormalSolver:
    """(A A')^-1 through a dense Cholesky: MFMA Gram for a DeviceDense A, sparse
    row products for a DeviceCSR A whose A A' is too wide for the banded
    solver; blocked Cholesky; explicit inverse applied as one matvec."""

    MAX_ROWS_FROM_SPARSE = 16384     # 2 GiB of G^-1

    def __init__(self, A):
        lib = _hip.load()
        m, n = A.shape
        self.m = m
        M = int(lib.ipx_dense_padded(m))
        dev = ctx().device
        G = torch.empty((M, M), dtype=_F64, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        st = stream_ptr()
        if isinstance(A, AugmentedDense):
            self._structured_gram(A, G, st)
        elif isinstance(A, DeviceDense):
            _gram(m, n, A.t, n, G, st)
        else:
            p = A.pattern
            _hip.call("ipx_aat_dense", m, _p(p.indptr), _p(p.indices), _p(A.val), _p(G), st)
        work = torch.empty(M + 1, dtype=_F64, device=dev)
        _hip.call("ipx_chol_factor", M, _p(G), _p(flag), _p(work), st)
        fl = int(flag.item())
        if fl & 4:
            raise np.linalg.LinAlgError("Singular Jacobian matrix: A A' is not positive definite")
        # bit 1 alone: every pivot positive, one lost 43 bits (numerically rank deficient):
        # ``projections`` takes the SVD exit when the matrix is small enough, else keeps this
        # factorization with its refinement steps (pivot_ratio below)
        self.ill_conditioned = bool(fl & 1)
        # Digits lost by the factorization (~1/cond(A)^2).  The reference's pivoted QR
        # (projections.py:175-233) loses cond(A), not cond(A)^2: for an ill-conditioned
        # Jacobian the least-squares and row-space operators get that back by refinement
        # steps against their own residuals (the null-space operator has the reference's
        # orthogonality-driven loop already).  None at the conditioning of the benchmarks.
        self.pivot_ratio = float(work[M].item())
        r = self.pivot_ratio
        self.refine_steps = 0 if r > 1e-3 else (1 if r > 1e-8 else (2 if r > 1e-11 else 3))
        X = torch.empty((M, M), dtype=_F64, device=dev)
        _hip.call("ipx_chol_inverse", M, _p(G), _p(X), st)
        self.M = M
        self.Ginv = DeviceDense(X)
        self._pad = torch.zeros(M, dtype=_F64, device=dev) if M != m else None

    @staticmethod
    def _structured_gram(A, G, st):
        """G = J J' + diag(0_{m_eq}, s*s) for A = [[J_eq, 0], [J_ineq, diag(s)]]: the Gram of A's
        first n columns (leading dimension n + m_ineq), then the slack squares on the diagonal
        -- taken from A itself, so G is a function of A alone.  A constant J keeps its Gram
        (``A.stack.gram0``) for the whole solve: one shift per refactorization."""
        m, N = A.shape
        n = A.n_vars
        s_ptr = A.t.data_ptr() + 8 * (A.m_eq * N + n)
        if A.stack.constant:
            G0 = A.stack.gram0
            if G0 is None:
                G0 = A.stack.gram0 = torch.empty_like(G)
                _gram(m, n, A.t, N, G0, st)
            _hip.call("ipx_gram_shift", m, A.m_eq, _p(G0), s_ptr, N + 1, _p(G), st)
        else:
            _gram(m, n, A.t, N, G, st)
            _hip.call("ipx_gram_shift", m, A.m_eq, None, s_ptr, N + 1, _p(G), st)

    def solve(self, w):
        if self._pad is None:
            return self.Ginv.gemv(w)
        self._pad[:self.m].copy_(w.t)
        return self.Ginv.gemv(DVec(self._pad))[:self.m].copy()


def _gram(m, n, A, lda, G, st):
    """G (padded M x M) = A[:, :n] A[:, :n]' for a row-major A with leading dimension lda."""
    lib = _hip.load()
    splits = int(lib.ipx_gram_splits(m, n))
    ws = torch.empty(int(lib.ipx_gram_ws_doubles(m, splits)), dtype=_F64, device=G.device) \
        if splits > 1 else None
    _hip.call("ipx_gram_f64_mfma_split", m, n, _p(A), lda, _p(G), _p(ws), splits, st)
