"""Pattern-level analysis of ``S = A A'`` (host, once per pattern) and the banded solver
(csrc/banded.hip): ``(A A')^-1`` for a sparse A whose ``A A'`` is banded with a half bandwidth of
at most ``ipx_banded_kmax()``, after a bandwidth-reducing row order found by the analysis.
"""
import ctypes

import numpy as np
import torch

from . import _hip
from . import device as dv
from .device import DVec, _p, stream_ptr, ctx

_F64 = torch.float64


class HostPattern:
    """What the symbolic analysis (``_Symbolic``) reads of a pattern, on the host."""

    def __init__(self, indptr, indices, shape):
        self.indptr_h = np.ascontiguousarray(indptr, dtype=np.int32)
        self.indices_h = np.ascontiguousarray(indices, dtype=np.int32)
        self.shape = (int(shape[0]), int(shape[1]))
        self.nnz = int(self.indptr_h[-1])


def half_bandwidth_of_aat(pattern):
    """Half bandwidth of ``A A'`` from the pattern of ``A`` alone, O(nnz): rows i and j couple
    iff they share a column, so it is the widest (last row - first row) of a column.  (Forming
    the product pattern for this, and trying a reordering of it, costs 0.1 s on the barrier
    problem's 1e6-row augmented Jacobian, whose band no ordering makes narrow.)"""
    k = getattr(pattern, "_ipx_aat_half_bw", None)
    if k is None:
        m, n = pattern.shape
        rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(pattern.indptr_h))
        cols = pattern.indices_h
        first, last = np.full(n, m, dtype=np.int64), np.full(n, -1, dtype=np.int64)
        last[cols] = rows                      # rows ascend: the last write is the last row
        first[cols[::-1]] = rows[::-1]         # ... and reversed, the first
        used = last >= 0
        k = int(np.max(last[used] - first[used])) if used.any() else 0
        pattern._ipx_aat_half_bw = k
    return k


class _Symbolic:
    """Pattern-level analysis of S = A A' (host, once per pattern)."""

    def __init__(self, pattern):
        import scipy.sparse as sps
        from scipy.sparse.csgraph import reverse_cuthill_mckee
        m, n = pattern.shape
        ones = np.ones(pattern.nnz, dtype=np.float32)
        B = sps.csr_matrix((ones, pattern.indices_h, pattern.indptr_h), shape=(m, n))
        S = sps.csr_matrix(B.dot(B.T))
        S.sort_indices()

        def half_bw(M):
            coo = M.tocoo()
            return int(np.max(np.abs(coo.row - coo.col))) if coo.nnz else 0

        self.k = half_bw(S)
        assert self.k == half_bandwidth_of_aat(pattern), (self.k, half_bandwidth_of_aat(pattern))
        self.perm = None
        if self.k > 1 and m > 2:
            perm = np.ascontiguousarray(reverse_cuthill_mckee(S, symmetric_mode=True),
                                        dtype=np.int32)
            k2 = half_bw(S[perm][:, perm])
            if k2 < self.k:
                self.k, self.perm = k2, perm
        self.m = m

    def __del__(self):
        # handles parked by BandedNormalSolver for the next factorization on this pattern
        for _, handle, _ in self.__dict__.get("_handle_pool", []):
            try:
                _hip.load().ipx_banded_destroy(ctypes.c_void_p(handle))
            except Exception:
                pass


_SYMBOLIC_ATTR = "_ipx_aat_symbolic"


def _symbolic_for(pattern):
    sym = getattr(pattern, _SYMBOLIC_ATTR, None)
    if sym is None:
        sym = _Symbolic(pattern)
        setattr(pattern, _SYMBOLIC_ATTR, sym)
    return sym


def share_analysis(host, pattern):
    """The device pattern of rows that were analysed as a host pattern takes the analysis over
    (the objects themselves: handles parked on the symbolic analysis stay in one pool)."""
    for name in (_SYMBOLIC_ATTR, "_ipx_aat_half_bw", "_ipx_border_split", "_ipx_link_split"):
        if name in host.__dict__:
            pattern.__dict__[name] = host.__dict__[name]
    return pattern


HANDLE_STATS = {"created": 0, "pooled": 0, "deferred": 0}     # banded handles (diagnostics)


class BandedNotDecoupled(NotImplementedError):
    """Half bandwidth 5..8 on a long band whose separator blocks do not decouple numerically
    (csrc/banded.hip ipx_banded_create: there is no compiled separator level for them)."""


class BandedNormalSolver:
    """(A A')^-1 for sparse A with banded A A' (half bandwidth <= kmax)."""

    def __init__(self, A, chunk=64, col_weights=None, deferred=None):
        """``col_weights`` (device tensor, one per column of A) factors
        ``A diag(w) A'`` instead (Schur complements, boxschur.py).  ``deferred`` (an object with
        a device tensor ``verdict``: the outer iteration's chain, sqp_chain.py): the blocking
        read that ends a factorization is left out when the handle's previous factorization was
        clean -- the same verdict is assumed, a kernel checks it on the device
        (``ipx_banded_status_deferred``) and the caller reads ``verdict`` with its next block
        (``self.pending`` until then; ``confirm`` reads it on its own)."""
        sym = _symbolic_for(A.pattern)
        kmax = _hip.load().ipx_banded_kmax()
        if sym.k > kmax:
            raise NotImplementedError(
                "A A' has half bandwidth %d after reordering; the device banded "
                "solver handles <= %d (no host fallback)" % (sym.k, kmax))
        self.m = sym.m
        self.k = max(sym.k, 1)
        dev = ctx().device
        self.perm = None
        if sym.perm is not None:
            self.perm = torch.from_numpy(sym.perm).to(dev)          # new row i = old row perm[i]
            inv = np.empty_like(sym.perm)
            inv[sym.perm] = np.arange(self.m, dtype=np.int32)
            self.iperm = torch.from_numpy(inv).to(dev)
        # handle + band storage are recycled per pattern: creating / destroying a handle is a
        # dozen hipMalloc / hipFree calls (~0.5 ms), more than the numeric refresh itself
        lib = _hip.load()
        self._sym = sym          # the pool's handles are destroyed with `sym`: keep it alive
        self._pool = sym.__dict__.setdefault("_handle_pool", [])
        self._key = (self.m, self.k, int(chunk))
        self.handle, self.band = None, None
        for i, (key, handle, band) in enumerate(self._pool):
            if key == self._key:
                self.handle, self.band = handle, band
                del self._pool[i]
                break
        HANDLE_STATS["pooled" if self.handle is not None else "created"] += 1
        if self.handle is None:
            self.band = torch.empty((self.k + 1) * self.m, dtype=_F64, device=dev)
            self.handle = lib.ipx_banded_create(self.m, self.k, int(chunk))
            if not self.handle:
                raise _hip.IpxError("ipx_banded_create failed (m=%d, k=%d)" % (self.m, self.k))
        p = A.pattern
        self.pending, self.ill_conditioned = False, False
        if deferred is not None and self.perm is None and self.k == 1:
            # the whole refresh behind one entry and in three launches where the handle
            # qualifies (csrc/banded.hip ipx_banded_refactor); 0: it does not, nothing enqueued
            rc = lib.ipx_banded_refactor(ctypes.c_void_p(self.handle), self.m, self.k,
                                         _p(p.indptr), _p(p.indices), _p(A.val), _p(col_weights),
                                         _p(self.band), deferred.verdict.data_ptr(), stream_ptr())
            if rc < 0:
                _hip.check(rc, "ipx_banded_refactor")
            if rc == 1:
                self.pending, self._verdict = True, deferred.verdict
                HANDLE_STATS["deferred"] += 1
                return
        _hip.call("ipx_aat_band_w", self.m, self.k, _p(p.indptr), _p(p.indices), _p(A.val),
                  _p(self.perm), _p(col_weights), _p(self.band), stream_ptr())
        _hip.call("ipx_banded_factor", ctypes.c_void_p(self.handle), _p(self.band), stream_ptr())
        if deferred is not None and lib.ipx_banded_status_deferred(
                ctypes.c_void_p(self.handle), deferred.verdict.data_ptr(), stream_ptr()) == 0:
            self.pending, self._verdict = True, deferred.verdict
            HANDLE_STATS["deferred"] += 1
            return
        rc = lib.ipx_banded_status(ctypes.c_void_p(self.handle), stream_ptr())
        if rc == -3:
            raise np.linalg.LinAlgError("Singular Jacobian matrix: A A' is not positive definite")
        # -6: every pivot positive but one lost 43 bits against its diagonal entry: numerically
        # rank deficient.  ``projections`` takes the reference's SVD exit when the matrix is
        # small enough for a dense SVD, and otherwise keeps this factorization (the reference's
        # sparse LU only bails on exact singularity) under the orthogonality-driven refinement
        self.ill_conditioned = rc == -6
        if rc == -6:
            rc = 0
        if rc == -5:
            raise BandedNotDecoupled("A A' (m=%d, half bandwidth %d): separator blocks of the "
                                     "partitioned factorization are coupled" % (self.m, self.k))
        _hip.check(rc, "ipx_banded_status")

    POOL_MAX = 4

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if not h:
            return
        pool = getattr(self, "_pool", None)
        try:
            if pool is not None and len(pool) < self.POOL_MAX:
                pool.append((self._key, h, self.band))       # next factorization on this pattern
            else:
                _hip.load().ipx_banded_destroy(ctypes.c_void_p(h))
        except Exception:
            pass

    def _gather(self, x, idx):
        out = dv._empty(len(x))
        _hip.call("ipx_gather", len(x), _p(x.t), _p(idx), None, None, _p(out), stream_ptr())
        return DVec(out)

    def solve(self, w):
        """v = (A A')^-1 w, in the caller's (unpermuted) row order."""
        if self.perm is not None:
            w = self._gather(w, self.perm)
        out = dv._empty(self.m)
        _hip.call("ipx_banded_solve", ctypes.c_void_p(self.handle), _p(w.t), _p(out), stream_ptr())
        v = DVec(out)
        if self.perm is not None:
            v = self._gather(v, self.iperm)
        return v
