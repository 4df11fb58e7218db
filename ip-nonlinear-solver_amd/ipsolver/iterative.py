"""``(A A')^-1`` without a factorization: preconditioned conjugate gradients on the device
(csrc/pcg.hip)."""
import ctypes
import time
from warnings import warn

import numpy as np
import torch

from . import _hip
from . import device as dv
from . import solver_options
from .banded import _symbolic_for
from .device import CSRPattern, DVec, DeviceCSR, _p, stream_ptr, ctx

_F64 = torch.float64


class PcgArgs(ctypes.Structure):
    """Mirror of ipx_pcg_args (include/ipx.h)."""
    _P, _I = ctypes.c_void_p, ctypes.c_int64
    _fields_ = [("m", _I), ("n", _I),
                ("A_rowptr", _P), ("A_colidx", _P), ("A_val", _P), ("A_tiles", _P), ("A_ntiles", _I),
                ("At_rowptr", _P), ("At_colidx", _P), ("At_val", _P), ("At_tiles", _P),
                ("At_ntiles", _I), ("dinv", _P), ("v", _P), ("r", _P), ("p", _P), ("Sp", _P),
                ("t", _P), ("state", _P), ("part1", _P), ("part2", _P), ("grid", _I),
                ("binv", _P), ("border", _P), ("nblk", _I), ("z", _P), ("part3", _P),
                ("rsum", _P), ("coarse_of", _P), ("goff", _P), ("ncoarse", _I),
                ("X", _P), ("ldx", _I), ("y", _P), ("partc", _P)]


def _host_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _aggregate_greedy(indptr, indices, cap):
    """(agg, number of aggregates) of the graph of a symmetric CSR pattern with sorted columns:
    ``ipx_aggregate_greedy`` (csrc/aggregate.hip; host code, include/ipx.h has the rule)."""
    indptr = np.ascontiguousarray(indptr, dtype=np.int32)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    agg = np.empty(len(indptr) - 1, dtype=np.int32)
    count = _hip.call("ipx_aggregate_greedy", len(agg), _host_ptr(indptr), _host_ptr(indices),
                      int(cap), _host_ptr(agg))
    return agg, int(count)


class _Aggregation:
    """Host graph work of the "compact" and "two-level" preconditioners, once per pattern: the
    rows of ``S = A A'`` in aggregates of at most ``block`` (the blocks), the blocks in groups of
    at most ``group`` (the coarse rows; the blocks themselves while there are no more than
    ``coarse_max`` of them), the blocks numbered so that a group's are consecutive.

    ``order``: the rows block by block, each block padded to ``block`` slots with -1;
    ``coarse_of``: the group of every row; ``goff``: the groups' block offsets."""

    def __init__(self, pattern, block, coarse_max, coarse_limit):
        import scipy.sparse as sps
        m, n = pattern.shape
        ones = np.ones(pattern.nnz, dtype=np.float32)
        B = sps.csr_matrix((ones, pattern.indices_h, pattern.indptr_h), shape=(m, n))
        S = sps.csr_matrix(B.dot(B.T))
        S.sort_indices()
        agg, nblk = _aggregate_greedy(S.indptr, S.indices, block)
        rows = np.arange(m)
        group_cap = max(1, -(-nblk // int(coarse_max)))
        while True:
            if group_cap == 1:
                group, ncoarse = np.arange(nblk, dtype=np.int32), nblk
            else:
                P = sps.csr_matrix((np.ones(m, dtype=np.float32), (rows, agg)), shape=(m, nblk))
                Q = sps.csr_matrix(P.T.dot(S).dot(P))          # the quotient graph P'SP
                Q.sort_indices()
                group, ncoarse = _aggregate_greedy(Q.indptr, Q.indices, group_cap)
            if ncoarse <= coarse_limit:       # (what the coarse kernel stages in LDS)
                break
            group_cap += 1
        by_group = np.argsort(group, kind="stable")            # new block number -> old
        renumber = np.empty(nblk, dtype=np.int32)
        renumber[by_group] = np.arange(nblk, dtype=np.int32)
        agg, group = renumber[agg], group[by_group]
        by_block = np.argsort(agg, kind="stable")              # rows ascending within a block
        sizes = np.bincount(agg, minlength=nblk)
        first = np.cumsum(sizes) - sizes
        order = np.full(nblk * block, -1, dtype=np.int32)
        order[agg[by_block] * block + (rows - np.repeat(first, sizes))] = by_block
        self.block, self.nblk, self.group, self.ncoarse = block, nblk, group_cap, int(ncoarse)
        self.agg, self.order = agg, order
        self.coarse_of = group[agg].astype(np.int32)
        self.goff = np.searchsorted(group, np.arange(ncoarse + 1)).astype(np.int32)
        # pattern of C = P'A: per group the union of its rows' columns
        Pc = sps.csr_matrix((np.ones(m, dtype=np.float32), (rows, self.coarse_of)),
                            shape=(m, ncoarse))
        C = sps.csr_matrix(Pc.T.dot(B))
        C.sort_indices()
        self.C_indptr, self.C_indices, self.C_shape = C.indptr, C.indices, (int(ncoarse), n)
        self._device = None

    def device(self):
        """``order``, ``coarse_of``, ``goff`` and the pattern of C in device memory (once)."""
        if self._device is None:
            dev = ctx().device
            up = lambda a: torch.from_numpy(a).to(dev)
            self._device = (up(self.order), up(self.coarse_of), up(self.goff),
                            CSRPattern(self.C_indptr, self.C_indices, self.C_shape))
        return self._device


def _aggregation_for(pattern, block, coarse_max):
    """The aggregation of a pattern, cached on it like the symbolic analysis (``_symbolic_for``):
    a factorization with new values on the same pattern does no host graph work."""
    cache = pattern.__dict__.setdefault("_ipx_aggregation", {})
    key = (int(block), int(coarse_max))
    if key not in cache:
        cache[key] = _Aggregation(pattern, key[0], key[1], _hip.load().ipx_pcg_coarse_max())
    return cache[key]


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
    on the device once per factorization; "jacobi" -- the diagonal (round 2).

    Opt-in, for matrices whose ``A A'`` is a graph Laplacian plus a shift (network flow,
    discretised PDE constraints), where the strips of the reverse Cuthill-McKee order are thin
    pieces of level sets: "compact" -- the same 32 x 32 blocks over aggregates grown breadth-first
    in the graph of ``A A'`` (``ipx_aggregate_greedy``); "two-level" -- those blocks plus the
    coarse correction ``P (P' A A' P)^-1 P'``, the columns of P the indicator vectors of the
    blocks (of groups of blocks past ``COARSE_MAX`` of them): ``C = P'A`` is assembled on the
    device and ``DenseNormalSolver(C)`` gives the explicit inverse, applied inside the loop by one
    more launch per iteration.  ``precond=None`` (default): the scoped solver option
    ``iterative_precond`` (solver_options.py), "block" unless set."""

    perm = None
    RTOL, MAXIT = 1e-15, 2000
    WARN_RELRES = 1e-10          # a solve that ends above this says so (warning)
    PS_RZ0, PS_BEST0, PS_DONE, PS_ITERS, PS_NORM_W, PS_RTOL, PS_STALL_FAR = 0, 2, 6, 7, 8, 9, 11
    STALL_FAR = 30               # iterations without a new smallest residual that end a solve
                                 # whose residual is still above 1e-9 ||w|| (5 below that)
    BLOCK = 32
    COARSE_MAX = 4096            # coarse rows: X = (C C')^-1 is at most 128 MB, read once per
                                 # iteration; more blocks than this are grouped
    PRECONDS = ("block", "compact", "two-level", "jacobi")

    def __init__(self, A, precond=None):
        lib = _hip.load()
        if precond is None:
            precond = solver_options.current().iterative_precond
        if precond not in self.PRECONDS:
            raise ValueError("precond must be one of %s, not %r"
                             % (", ".join(repr(p) for p in self.PRECONDS), precond))
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
        self.blocks = self.coarse_rows = self.group = 0
        # host seconds of the build's stages (each ends in a blocking read): the row order (the
        # symbolic analysis or the aggregation: host graph work on a pattern's first build
        # only), the blocks, the coarse level
        clock = [time.perf_counter()]
        if precond != "jacobi":
            if precond == "block":
                # rows in the order of the symbolic analysis, padded to whole blocks
                order = _symbolic_for(A.pattern).perm
                order = np.arange(m, dtype=np.int32) if order is None \
                    else np.asarray(order, np.int32)
                nblk = (m + self.BLOCK - 1) // self.BLOCK
                padded = np.full(nblk * self.BLOCK, -1, dtype=np.int32)
                padded[:m] = order
                self.border = torch.from_numpy(padded).to(dev)
            else:
                # aggregates of the graph of A A', each padded to a whole block
                self.aggregation = _aggregation_for(A.pattern, self.BLOCK, self.COARSE_MAX)
                nblk = self.aggregation.nblk
                self.border = self.aggregation.device()[0]
            self.blocks = nblk
            clock.append(time.perf_counter())
            self.binv = torch.empty(nblk * self.BLOCK * self.BLOCK, dtype=_F64, device=dev)
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            pat = A.pattern
            _hip.call("ipx_blockjacobi_build", nblk, _p(pat.indptr), _p(pat.indices), _p(A.val),
                      _p(self.border), _p(self.binv), _p(flag), stream_ptr())
            fl = int(flag.item())
            clock.append(time.perf_counter())
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
        if precond == "two-level":
            self._build_coarse(A)
            clock.append(time.perf_counter())
        self.build_seconds = dict(zip(("order", "blocks", "coarse"), np.diff(clock)))
        self.stats = {"solves": 0, "iterations": 0, "batches": 0, "blocks": self.blocks,
                      "coarse_rows": self.coarse_rows, "group": self.group}

    def _build_coarse(self, A):
        """The coarse level: C = P'A on the device (``ipx_csr_aggregate_rows``), the explicit
        inverse of C C' = P' A A' P from the dense solver."""
        from .dense import DenseNormalSolver
        lib, a, ag = _hip.load(), self.args, self.aggregation
        _, coarse_of, goff, Cpat = ag.device()
        dev, nc = ctx().device, ag.ncoarse
        Cval = torch.empty(Cpat.nnz, dtype=_F64, device=dev)
        pat = A.pattern
        _hip.call("ipx_csr_aggregate_rows", nc, _p(pat.indptr), _p(pat.indices), _p(A.val),
                  _p(self.border), _p(goff), _p(Cpat.indptr), _p(Cpat.indices), _p(Cval),
                  stream_ptr())
        self.C = DeviceCSR(Cpat, Cval)
        try:
            self.coarse = DenseNormalSolver(self.C)
        except np.linalg.LinAlgError:
            raise np.linalg.LinAlgError("Singular Jacobian matrix: the coarse matrix P' A A' P "
                                        "is not positive definite")
        self.ill_conditioned = self.ill_conditioned or self.coarse.ill_conditioned
        self.coarse_rows, self.group = nc, ag.group
        z = lambda k: torch.zeros(int(k), dtype=_F64, device=dev)
        self.rsum, self.y = z(self.blocks), z(nc)
        self.partc, self.rz = z(lib.ipx_pcg_coarse_grid(nc)), z(1)
        self._coarse_of, self._goff = coarse_of, goff
        a.rsum, a.coarse_of, a.goff = self.rsum.data_ptr(), coarse_of.data_ptr(), goff.data_ptr()
        a.ncoarse, a.X, a.ldx = nc, self.coarse.Ginv.t.data_ptr(), self.coarse.M
        a.y, a.partc = self.y.data_ptr(), self.partc.data_ptr()

    def precond_apply(self, r):
        """(z, r'z) with ``z = M^-1 r`` of the two-level preconditioner (``ipx_pcg_precond_apply``;
        r a DVec, z this solver's buffer)."""
        self.state.zero_()
        _hip.call("ipx_pcg_precond_apply", ctypes.byref(self.args), _p(r.t), _p(self.z),
                  _p(self.rz), stream_ptr())
        return DVec(self.z), float(self.rz.item())

    def solve(self, w):
        lib = _hip.load()
        v = DVec.zeros(self.m)
        norm_w = dv.norm(w)
        if norm_w == 0:
            return v
        self.r.copy_(w.t)
        init = np.zeros(self.state.numel())
        rz0 = None
        if self.precond == "two-level":
            z0, rz0 = self.precond_apply(w)
        elif self.precond in ("block", "compact"):
            self.state.zero_()
            _hip.call("ipx_blockjacobi_apply", self.m, self.args.nblk, _p(self.border),
                      _p(self.binv), _p(w.t), _p(self.z), _p(self.part3), _p(self.state),
                      stream_ptr())
            z0 = DVec(self.z)
        else:
            z0 = self.dinv * w
        self.p.copy_(z0.t)
        init[self.PS_RZ0] = w.dot(z0) if rz0 is None else rz0
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
