"""``(A A')^-1`` for sparse A of any pattern by a sparse Cholesky factorization: nested dissection,
a supernodal multifrontal factorization and level-by-level triangular solves on the device
(csrc/nested_order.hip: the host graph work; csrc/nested.hip: the kernels).

Networks, unstructured meshes, power-flow style Jacobians: ``A A'`` has no band, and past the
dense Cholesky's 16384 rows the default is the preconditioned CG (iterative.py), whose accuracy
depends on the conditioning.  Opt-in (``projector.sparse_direct("nested-dissection")``,
``options={"sparse_direct": "nested-dissection"}``); the default selection is unchanged.
"""
import ctypes
import time

import numpy as np
import torch

from . import _hip
from . import device as dv
from . import solver_options
from .device import DVec, _p, stream_ptr, ctx

_P, _I64 = ctypes.c_void_p, ctypes.c_int64
ND_FIELDS = 12          # IPX_ND_FIELDS


class NdArgs(ctypes.Structure):
    """Mirror of ipx_nd_args (include/ipx.h)."""
    _fields_ = [("m", _I64), ("nsuper", _I64)] + \
               [(k, _P) for k in ("sn", "perm", "bnd_rows", "cmap", "child_idx", "lists",
                                  "A_rowptr", "A_colidx", "A_val", "fronts", "work", "y", "upd",
                                  "flag")]


class NestedDissectionRefused(NotImplementedError):
    """The matrix is past a limit of the nested-dissection solver (the message names it)."""


def _host_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class _NdSymbolic:
    """Host graph work, once per pattern and leaf size: the nested-dissection order of the graph
    of ``S = A A'`` (``ipx_nd_order``) and the supernodal symbolic factorization
    (``ipx_nd_symbolic``).  Positions are places in the new order; ``perm[position] = row``."""

    def __init__(self, pattern, leaf):
        import scipy.sparse as sps
        m, n = pattern.shape
        ones = np.ones(pattern.nnz, dtype=np.float32)
        B = sps.csr_matrix((ones, pattern.indices_h, pattern.indptr_h), shape=(m, n))
        S = sps.csr_matrix(B.dot(B.T))
        S.sort_indices()
        indptr = np.ascontiguousarray(S.indptr, dtype=np.int32)
        indices = np.ascontiguousarray(S.indices, dtype=np.int32)
        perm = np.empty(m, dtype=np.int32)
        sn_ptr = np.empty(m + 1, dtype=np.int32)
        ns = int(_hip.call("ipx_nd_order", m, _host_ptr(indptr), _host_ptr(indices), int(leaf),
                           _host_ptr(perm), _host_ptr(sn_ptr)))
        sn_ptr = sn_ptr[:ns + 1].copy()
        parent = np.empty(ns, dtype=np.int32)
        level = np.empty(ns, dtype=np.int32)
        bnd_ptr = np.empty(ns + 1, dtype=np.int64)
        symbolic = lambda bnd, cmap, cap: _hip.call(
            "ipx_nd_symbolic", m, _host_ptr(indptr), _host_ptr(indices), ns, _host_ptr(perm),
            _host_ptr(sn_ptr), _host_ptr(parent), _host_ptr(level), _host_ptr(bnd_ptr), bnd, cmap,
            cap)
        total = int(symbolic(None, None, 0))
        bnd = np.empty(max(total, 1), dtype=np.int32)
        cmap = np.zeros(max(total, 1), dtype=np.int32)
        symbolic(_host_ptr(bnd), _host_ptr(cmap), total)
        self.m, self.leaf, self.nsuper = m, int(leaf), ns
        self.perm, self.sn_ptr, self.parent, self.level = perm, sn_ptr, parent, level
        self.bnd_ptr, self.bnd, self.cmap = bnd_ptr, bnd[:total], cmap[:total]
        self.own = np.diff(sn_ptr).astype(np.int64)              # s of every supernode
        self.boundary = np.diff(bnd_ptr)                         # b
        self.largest_front = int((self.own + self.boundary).max()) if ns else 0
        self.levels = int(level.max()) + 1 if ns else 0
        self.plans = {}


def _analyze(pattern, leaf):
    return _NdSymbolic(pattern, leaf)


def _nd_symbolic_for(pattern, leaf):
    """The analysis of a pattern, cached on it like ``_symbolic_for`` / ``_aggregation_for``: a
    factorization with new values on the same pattern does no host graph work."""
    cache = pattern.__dict__.setdefault("_ipx_nested", {})
    if int(leaf) not in cache:
        cache[int(leaf)] = _analyze(pattern, int(leaf))
    return cache[int(leaf)]


class _Plan:
    """Where every front lives and what every launch takes, for one cut between small and large
    fronts: the table ``sn`` of include/ipx.h, the level lists (per level the small fronts, then
    the large ones), the byte counts.  Host arrays; ``device()`` uploads them once."""

    def __init__(self, sym, small_front):
        s, b = sym.own, sym.boundary
        f = s + b
        ns = sym.nsuper
        small = f <= small_front
        pad = np.where(small, 0, (-s) % 64)
        ld = np.where(small, f, -(-(s + pad + b) // 64) * 64)
        size = ld * ld
        work = np.where(small, 0, ld + 1)
        has = sym.parent >= 0
        kids = np.flatnonzero(has)
        kids = kids[np.argsort(sym.parent[kids], kind="stable")]   # by parent, ascending within
        nkids = np.bincount(sym.parent[has], minlength=ns)
        sn = np.zeros((ns, ND_FIELDS), dtype=np.int64)
        sn[:, 0], sn[:, 1], sn[:, 2] = sym.sn_ptr[:-1], s, b
        sn[:, 3] = sym.bnd_ptr[:-1]
        sn[:, 4] = np.cumsum(size) - size
        sn[:, 5], sn[:, 6] = ld, pad
        sn[:, 8] = np.cumsum(nkids)
        sn[:, 7] = sn[:, 8] - nkids
        sn[:, 9] = np.cumsum(work) - work
        self.sn, self.child_idx = sn, kids.astype(np.int32)
        # the level lists: (level, large, number) ascending
        order = np.lexsort((np.arange(ns), ~small, sym.level))
        self.lists = order.astype(np.int32)
        self.levels = []                 # (offset, small fronts, their largest, large, largest)
        at = 0
        for lv in range(sym.levels):
            here = order[at:at + int(np.sum(sym.level == lv))]
            nsm = int(small[here].sum())
            fmax = lambda idx: int(f[idx].max()) if len(idx) else 0
            self.levels.append((at, nsm, fmax(here[:nsm]), len(here) - nsm, fmax(here[nsm:])))
            at += len(here)
        # what a solve's launches take: (offset, fronts, the largest front) per level
        self.solve_levels = np.array([(at, nsm + nlg, max(fsm, flg))
                                      for at, nsm, fsm, nlg, flg in self.levels],
                                     dtype=np.int64).reshape(-1, 3)
        self.front_doubles, self.work_doubles = int(size.sum()), int(work.sum())
        self.factor_bytes = int(8 * (s * (s + 1) // 2 + b * s).sum())
        ints = sym.m + 2 * len(sym.bnd) + len(self.lists) + len(self.child_idx)
        self.doubles = self.front_doubles + self.work_doubles + sym.m + len(sym.bnd)
        self.bytes = 8 * self.doubles + 4 * ints + 8 * sn.size
        self.large_fronts = int((~small).sum())
        self._device = None

    def device(self, sym):
        if self._device is None:
            dev = ctx().device
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            self._device = {"sn": up(self.sn.ravel()), "perm": up(sym.perm),
                            "bnd_rows": up(sym.perm[sym.bnd] if len(sym.bnd) else sym.bnd),
                            "cmap": up(sym.cmap), "child_idx": up(self.child_idx),
                            "lists": up(self.lists)}
        return self._device


class NestedDissectionNormalSolver:
    """(A A')^-1 by a multifrontal Cholesky factorization of ``P A A' P'``, P a nested-dissection
    order.  Fronts of at most ``SMALL_FRONT`` rows are factored by one workgroup each out of LDS,
    a tree level per launch; larger ones by 64 x 64 tiles on the fp64 matrix cores.  A solve is
    one launch per tree level forward and one backward; it is in the caller's row order, and
    bit-identical from run to run."""

    LEAF = 64                    # a part of at most this many rows is not dissected further
    SMALL_FRONT = 128            # the cut between the two paths (at most ipx_nd_small_max())
    FRONT_MAX = 2048             # no front larger than this
    MAX_BYTES = 2 << 30          # device storage: fronts (factor and updates), vectors, tables
    _FACTOR = ("ipx_nd_factor_small", "ipx_nd_factor_large")    # the entry of either path

    def __init__(self, A):
        lib = _hip.load()
        clock = time.perf_counter()
        sym = self.symbolic = _nd_symbolic_for(A.pattern, self.LEAF)
        self.analysis_seconds = time.perf_counter() - clock
        self.m = sym.m
        if sym.largest_front > self.FRONT_MAX:
            raise NestedDissectionRefused(
                "the nested-dissection order of A A' has a front of %d rows; the solver handles "
                "<= %d" % (sym.largest_front, self.FRONT_MAX))
        cut = min(int(self.SMALL_FRONT), int(lib.ipx_nd_small_max()))
        plan = sym.plans.get(cut)
        if plan is None:
            plan = sym.plans[cut] = _Plan(sym, cut)
        self.plan = plan
        if plan.bytes > self.MAX_BYTES:
            raise NestedDissectionRefused(
                "the multifrontal factorization of A A' needs %d bytes of device storage; the "
                "solver takes <= %d" % (plan.bytes, self.MAX_BYTES))
        dev = ctx().device
        d = self._tables = plan.device(sym)
        # one tensor owns everything the factorization and the solves use
        self.ws = torch.zeros(plan.doubles, dtype=torch.float64, device=dev)
        self.flag = torch.zeros(2, dtype=torch.int32, device=dev)
        base, a = self.ws.data_ptr(), NdArgs()
        a.m, a.nsuper = sym.m, sym.nsuper
        for k, t in d.items():
            setattr(a, k, t.data_ptr())
        pat = A.pattern
        a.A_rowptr, a.A_colidx, a.A_val = pat.indptr.data_ptr(), pat.indices.data_ptr(), \
            A.val.data_ptr()
        a.fronts = base
        a.work = base + 8 * plan.front_doubles
        a.y = a.work + 8 * plan.work_doubles
        a.upd = a.y + 8 * sym.m
        a.flag = self.flag.data_ptr()
        self.args, self._A = a, A
        self.stats = {"solves": 0, "levels": sym.levels, "fronts": sym.nsuper,
                      "largest_front": sym.largest_front, "large_fronts": plan.large_fronts,
                      "factor_bytes": plan.factor_bytes, "storage_bytes": plan.bytes,
                      "launches_per_solve": 2 * sym.levels}
        self._factor()

    def _level(self, lv, assemble_only=0):
        a, st, plan = ctypes.byref(self.args), stream_ptr(), self.plan
        at, nsm, fsm, nlg, _ = plan.levels[lv]
        if nsm:
            _hip.call(self._FACTOR[0], a, at, nsm, fsm, assemble_only, st)
        if nlg:
            _hip.call(self._FACTOR[1], a, _host_ptr(plan.sn), _host_ptr(plan.lists),
                      at + nsm, nlg, assemble_only, st)

    def assemble_level(self, lv):
        """The fronts of tree level ``lv`` as assembled -- the entries of S and the updates of
        their (factored) children --, not factored: for the tests, read with ``front``.  The
        factorization is void afterwards."""
        self._level(lv, assemble_only=1)

    def _factor(self):
        for lv in range(len(self.plan.levels)):
            self._level(lv)
        bits = int(self.flag[0].item())
        if bits & 4:
            raise np.linalg.LinAlgError("Singular Jacobian matrix: A A' is not positive definite")
        # bit 0 alone: every pivot positive, one lost 43 bits against its diagonal entry --
        # ``projections`` takes its SVD-or-warn exit
        self.ill_conditioned = bool(bits & 1)
        self.flag_bits = bits

    def front(self, j):
        """Front j as the factorization left it (host array, its storage rows and columns)."""
        off, ld = int(self.plan.sn[j, 4]), int(self.plan.sn[j, 5])
        return self.ws[off:off + ld * ld].reshape(ld, ld).cpu().numpy()

    def solve(self, w):
        """v = (A A')^-1 w, in the caller's row order."""
        out = dv._empty(self.m)
        table = self.plan.solve_levels
        _hip.call("ipx_nd_solve", ctypes.byref(self.args), len(table), _host_ptr(table),
                  _p(w.t), _p(out), stream_ptr())
        self.stats["solves"] += 1
        return DVec(out)


class PivotSkippingNestedSolver(NestedDissectionNormalSolver):
    """The same factorization in skip mode, for a rank-deficient A: a pivot within 2^-43 of its
    diagonal entry of zero is a row of A that depends on the rows eliminated before it (or a zero
    row); it is dropped -- a zero column of L under a diagonal stored as +inf.  What is factored is
    ``A_S A_S'``, S the kept rows, and ``solve(w)`` returns ``(A_S A_S')^-1 w_S`` on S and exactly
    0 on the dropped rows, whatever ``w`` holds there (the solve kernels divide by the diagonal:
    x / inf = 0).  ``dropped``: the dropped rows, ascending (host); ``rank = m - len(dropped)``;
    ``mark``: 1 at a dropped row (device int32).  The analysis, the plan and the limits
    (``NestedDissectionRefused``) are the base class's; a negative pivot or a NaN is still
    ``LinAlgError``."""

    _FACTOR = ("ipx_nd_factor_small_skip", "ipx_nd_factor_large_skip")

    def _factor(self):
        NestedDissectionNormalSolver._factor(self)
        self.mark = torch.empty(self.m, dtype=torch.int32, device=self.ws.device)
        _hip.call("ipx_nd_skipped", ctypes.byref(self.args), _p(self.mark), stream_ptr())
        self.dropped = np.flatnonzero(self.mark.cpu().numpy()).astype(np.int32)   # (the one read)
        self.rank = self.m - len(self.dropped)
        self.stats["dropped"] = len(self.dropped)


def nested_dissection_solver(A):
    """The nested-dissection solver of A under the option ``sparse_direct``, or None: the option
    is off, or the matrix is past the solver's limits (``NestedDissectionRefused``)."""
    if solver_options.current().sparse_direct != "nested-dissection":
        return None
    try:
        return NestedDissectionNormalSolver(A)
    except NestedDissectionRefused:
        return None
