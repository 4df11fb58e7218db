"""``(A A')^-1`` for sparse A whose ``A A'`` has a half bandwidth past the banded solver's and
up to 64: block cyclic reduction of the block-tridiagonal matrix (csrc/blocktri.hip).

Discretised dynamics (optimal control, collocation, multi-stage problems) with d states per
stage give ``J J'`` block tridiagonal in blocks of d, half bandwidth 2 d - 1: past the banded
kernels from d = 5 on, and past the dense Cholesky from 16384 rows on.  Opt-in
(``projector.wide_band("block-tridiagonal")``, ``options={"wide_band": ...}``); the default
policy keeps the preconditioned CG for such matrices.
"""
import ctypes

import numpy as np
import torch

from . import _hip
from . import device as dv
from .banded import _symbolic_for
from .device import DVec, _p, stream_ptr, ctx

BLOCK_SIZES = (16, 32, 64)     # (the largest is ipx_blocktri_kmax())


def block_size(k):
    """The block edge for half bandwidth k: the smallest of 16, 32, 64 with b >= k (k <= b is
    exactly the condition for block tridiagonality)."""
    for b in BLOCK_SIZES:
        if k <= b:
            return b
    raise NotImplementedError("A A' has half bandwidth %d after reordering; the block-tridiagonal "
                              "solver handles <= %d" % (k, BLOCK_SIZES[-1]))


class BlockTridiagonalNormalSolver:
    """(A A')^-1 by block cyclic reduction; pivot blocks applied as triangular factors."""

    _ABI = "blocktri"       # the entry points are ipx_<_ABI>_factor, ipx_aat_<_ABI>, ...
    _NAME = "block-tridiagonal"
    _block_size = staticmethod(block_size)

    def __init__(self, A):
        lib = _hip.load()
        abi = self._ABI
        sym = _symbolic_for(A.pattern)
        kmax = getattr(lib, "ipx_%s_kmax" % abi)()
        if sym.k > kmax:
            raise NotImplementedError(
                "A A' has half bandwidth %d after reordering; the %s solver "
                "handles <= %d" % (sym.k, self._NAME, kmax))
        self.m = sym.m
        self.k = max(sym.k, 1)
        self.b = self._block_size(self.k)
        dev = ctx().device
        self.perm = None
        if sym.perm is not None:
            self.perm = torch.from_numpy(sym.perm).to(dev)          # new row i = old row perm[i]
            inv = np.empty_like(sym.perm)
            inv[sym.perm] = np.arange(self.m, dtype=np.int32)
            self.iperm = torch.from_numpy(inv).to(dev)
        m, b = self.m, self.b
        nblk = -(-m // b)
        # one tensor owns everything the factorization and the solves use (include/ipx.h)
        self.ws = torch.empty(int(getattr(lib, "ipx_%s_ws_doubles" % abi)(m, b)),
                              dtype=torch.float64, device=dev)
        flag = torch.zeros(2, dtype=torch.int32, device=dev)
        D = ctypes.c_void_p(self.ws.data_ptr())
        E = ctypes.c_void_p(self.ws.data_ptr() + 8 * nblk * b * b)
        p = A.pattern
        _hip.call("ipx_aat_%s" % abi, m, b, self.k, _p(p.indptr), _p(p.indices), _p(A.val),
                  _p(self.perm), D, E, stream_ptr())
        _hip.call("ipx_%s_factor" % abi, m, b, D, E, _p(self.ws), _p(flag), stream_ptr())
        geo = (ctypes.c_int32 * 2)()
        self.level_launches = int(_hip.call("ipx_%s_levels" % abi, m, b, geo))
        bits = int(flag[0].item())
        if bits & 4:
            raise np.linalg.LinAlgError("Singular Jacobian matrix: A A' is not positive definite")
        # bit 0 alone: every pivot positive, one lost 43 bits against its diagonal entry --
        # ``projections`` takes its SVD-or-warn exit
        self.ill_conditioned = bool(bits & 1)
        self.flag_bits = bits
        self.stats = {"solves": 0, "levels": int(geo[0])}

    def _gather(self, x, idx):
        out = dv._empty(len(x))
        _hip.call("ipx_gather", len(x), _p(x.t), _p(idx), None, None, _p(out), stream_ptr())
        return DVec(out)

    def solve(self, w):
        """v = (A A')^-1 w, in the caller's (unpermuted) row order."""
        if self.perm is not None:
            w = self._gather(w, self.perm)
        out = dv._empty(self.m)
        _hip.call("ipx_%s_solve" % self._ABI, self.m, self.b, _p(self.ws), _p(w.t), _p(out),
                  stream_ptr())
        self.stats["solves"] += 1
        v = DVec(out)
        if self.perm is not None:
            v = self._gather(v, self.iperm)
        return v
