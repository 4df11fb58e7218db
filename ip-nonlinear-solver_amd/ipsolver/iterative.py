"""``(A A')^-1`` without a factorization: preconditioned conjugate gradients on the device
(csrc/pcg.hip)."""
import ctypes
from warnings import warn

import numpy as np
import torch

from . import _hip
from . import device as dv
from .banded import _symbolic_for
from .device import DVec, DeviceCSR, _p, stream_ptr, ctx

_F64 = torch.float64


class PcgArgs(ctypes.Structure):
    """Mirror of ipx_pcg_args (include/ipx.h)."""
    _P, _I = ctypes.c_void_p, ctypes.c_int64
    _fields_ = [("m", _I), ("n", _I),
                ("A_rowptr", _P), ("A_colidx", _P), ("A_val", _P), ("A_tiles", _P), ("A_ntiles", _I),
                ("At_rowptr", _P), ("At_colidx", _P), ("At_val", _P), ("At_tiles", _P),
                ("At_ntiles", _I), ("dinv", _P), ("v", _P), ("r", _P), ("p", _P), ("Sp", _P),
                ("t", _P), ("state", _P), ("part1", _P), ("part2", _P), ("grid", _I),
                ("binv", _P), ("border", _P), ("nblk", _I), ("z", _P), ("part3", _P)]


class IterativeNormalSolver:
    """``(A A')^-1`` without a factorization, for sparse Jacobians whose ``A A'`` is neither
    banded (after reordering) nor small enough for the dense device Cholesky: preconditioned
    conjugate gradients on ``A (A' v) = w``, device resident (csrc/pcg.hip):
    one C call enqueues a batch of iterations, convergence and stall tests are taken on the
    device, the host reads one state block per batch.  The reference factors any sparse A
    with SuperLU (projections.py:93-172); this keeps such problems solvable here (at the
    speed of an iterative solve) instead of refusing them.  The inner solve runs to the
    floor of fp64; the projector's orthogonality-driven refinement (projections.py:72-78)
    sits on top of it as usual.

    Preconditioner (``precond``): "block" (default) -- block Jacobi: the diagonal 32 x 32 blocks
    of ``A A'`` with the rows taken in the bandwidth-reducing order of the symbolic analysis
    (reverse Cuthill-McKee of the pattern of ``A A'``), formed, Cholesky-factored and inverted
    on the device once per factorization; "jacobi" -- the diagonal (round 2)."""

    perm = None
    RTOL, MAXIT = 1e-15, 2000
    WARN_RELRES = 1e-10          # a solve that ends above this says so (warning)
    PS_RZ0, PS_BEST0, PS_DONE, PS_ITERS, PS_NORM_W, PS_RTOL, PS_STALL_FAR = 0, 2, 6, 7, 8, 9, 11
    STALL_FAR = 30               # iterations without a new smallest residual that end a solve
                                 # whose residual is still above 1e-9 ||w|| (5 below that)
    BLOCK = 32

    def __init__(self, A, precond="block"):
        lib = _hip.load()
        self.precond = precond
        self.A, self.At = A, A.T
        self.m, n = A.shape
        sq = DVec(A.val) * DVec(A.val)
        rowsq = DeviceCSR(A.pattern, sq.t).dot(DVec.full(n, 1.0))
        d = rowsq.to_host()
        if not np.all(d > 0):
            raise np.linalg.LinAlgError("Singular Jacobian matrix: a row of A is zero")
        self.dinv = DVec.from_host(1.0 / d)
        dev, m = ctx().device, self.m
        z = lambda k: torch.zeros(int(k), dtype=_F64, device=dev)
        self.r, self.p, self.Sp, self.t = z(m), z(m), z(m), z(n)
        self.state = z(lib.ipx_pcg_state_size())
        self.grid = int(lib.ipx_cg_vec_grid(max(m, 1)))
        self.part1, self.part2 = z(2 * A.pattern.ntiles), z(2 * self.grid)
        a = self.args = PcgArgs()
        a.m, a.n = m, n
        for pre, M in (("A", A), ("At", self.At)):
            pat = M.pattern
            setattr(a, pre + "_rowptr", pat.indptr.data_ptr())
            setattr(a, pre + "_colidx", pat.indices.data_ptr())
            setattr(a, pre + "_val", M.val.data_ptr())
            setattr(a, pre + "_tiles", pat.tiles.data_ptr())
            setattr(a, pre + "_ntiles", pat.ntiles)
        a.dinv = self.dinv.t.data_ptr()
        a.r, a.p, a.Sp, a.t = (t.data_ptr() for t in (self.r, self.p, self.Sp, self.t))
        a.state, a.part1, a.part2 = (t.data_ptr() for t in (self.state, self.part1, self.part2))
        a.grid = self.grid
        if precond == "block":
            # rows in the order of the symbolic analysis, padded to whole blocks
            order = _symbolic_for(A.pattern).perm
            order = np.arange(m, dtype=np.int32) if order is None else np.asarray(order, np.int32)
            nblk = (m + self.BLOCK - 1) // self.BLOCK
            padded = np.full(nblk * self.BLOCK, -1, dtype=np.int32)
            padded[:m] = order
            self.border = torch.from_numpy(padded).to(dev)
            self.binv = torch.empty(nblk * self.BLOCK * self.BLOCK, dtype=_F64, device=dev)
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            pat = A.pattern
            _hip.call("ipx_blockjacobi_build", nblk, _p(pat.indptr), _p(pat.indices), _p(A.val),
                      _p(self.border), _p(self.binv), _p(flag), stream_ptr())
            fl = int(flag.item())
            if fl & 1:
                raise np.linalg.LinAlgError("Singular Jacobian matrix: a diagonal block of A A' "
                                            "is not positive definite")
            # bit 2 alone: every pivot positive, one lost 43 bits (a block numerically rank
            # deficient); the solve goes on, as with the dense factorization
            self.ill_conditioned = bool(fl & 2)
            self.z, self.part3 = z(m), z(nblk // 8 + 2)
            self.dinv = DVec.zeros(m)             # (r'z comes from the block kernel)
            a.dinv = self.dinv.t.data_ptr()
            a.binv, a.border, a.nblk = self.binv.data_ptr(), self.border.data_ptr(), nblk
            a.z, a.part3 = self.z.data_ptr(), self.part3.data_ptr()
        elif precond != "jacobi":
            raise ValueError("precond must be 'block' or 'jacobi'")
        self.stats = {"solves": 0, "iterations": 0, "batches": 0}

    def solve(self, w):
        lib = _hip.load()
        v = DVec.zeros(self.m)
        norm_w = dv.norm(w)
        if norm_w == 0:
            return v
        self.r.copy_(w.t)
        init = np.zeros(self.state.numel())
        if self.precond == "block":
            self.state.zero_()
            _hip.call("ipx_blockjacobi_apply", self.m, self.args.nblk, _p(self.border),
                      _p(self.binv), _p(w.t), _p(self.z), _p(self.part3), _p(self.state),
                      stream_ptr())
            z0 = DVec(self.z)
        else:
            z0 = self.dinv * w
        self.p.copy_(z0.t)
        init[self.PS_RZ0] = w.dot(z0)
        init[self.PS_BEST0] = np.inf
        init[self.PS_NORM_W], init[self.PS_RTOL] = norm_w, self.RTOL
        init[self.PS_STALL_FAR] = self.STALL_FAR
        self.state.copy_(torch.from_numpy(init))
        self.args.v = v.t.data_ptr()
        it, batch = 0, 8
        while it < self.MAXIT:
            end = min(self.MAXIT, it + batch)
            _hip.check(lib.ipx_pcg_iterate(ctypes.byref(self.args), it, end, stream_ptr()),
                       "ipx_pcg_iterate")
            s = self.state.tolist()               # one blocking read per batch
            self.stats["batches"] += 1
            if s[self.PS_DONE] != 0:
                if s[self.PS_DONE] == 3:
                    raise np.linalg.LinAlgError("Singular Jacobian matrix: A A' is not positive "
                                                "definite")
                break
            it, batch = end, min(2 * batch, 64)
        self.stats["solves"] += 1
        self.stats["iterations"] += int(s[self.PS_ITERS])
        # neither converged nor down at the floor of fp64 (MAXIT reached, or no progress far
        # above it): the reference's direct factorization would have been accurate here --
        # say so instead of returning a poor solve silently
        relres = min(s[self.PS_BEST0], s[self.PS_BEST0 + 1]) / norm_w
        self.stats["worst_relres"] = max(self.stats.get("worst_relres", 0.0), relres)
        if s[self.PS_DONE] != 1 and relres > self.WARN_RELRES:
            warn("IterativeNormalSolver: the preconditioned CG on A A' stopped at a relative "
                 "residual of %.1e after %d iterations (ill-conditioned Jacobian; m = %d): "
                 "projections with this factorization are only that accurate"
                 % (relres, int(s[self.PS_ITERS]), self.m))
        return v
