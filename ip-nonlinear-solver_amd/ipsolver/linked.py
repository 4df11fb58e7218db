"""``(A A')^-1`` for a sparse A that is banded / block tridiagonal in ``A A'`` but for a few dense
rows (csrc/linked.hip): staged problems with linking constraints -- a fuel or energy budget over
all stages, a periodicity condition ``x_N = x_0``, an average, a terminal bound that sees every
stage.

The rows of A are band rows B and q <= 32 link rows D, in any positions of the caller's order:

    S = A A' = [ S_B  E ]     S_B = B B',  E = B D',  F = D D',
               [ E'   F ]
    Y = S_B^-1 E,   K = F - E' Y,   u = S_B^-1 w_B,   K z = w_D - Y' w_B,   v_B = u - Y z,  v_D = z,

one solve with the direct factorization of ``S_B`` (``BorderedNormalSolver``,
``BandedNormalSolver``, ``BlockTridiagonalNormalSolver`` or its wide form, unchanged) plus O(m q)
work.  Opt-in:
``projector.link_rows(limit)``, ``options={"link_rows": limit}``.

This is a block Cholesky of an SPD matrix, not a Woodbury update: its error carries
``kappa(S_B)`` and not the cancellation in K, so there is no growth guard
and no refinement step here.  The solver refuses (``LinkedRefused``) when the inner solver fails
or reports ``ill_conditioned`` or when K has a non-positive pivot, and reports
``ill_conditioned`` when a pivot of K falls below 2^-43 of its ``F_jj`` -- the diagonal entry of
S, as for the other solvers.  ``cancellation`` (max_j F_jj / K_jj) is a diagnostic.
"""
import numpy as np
import torch

from . import _hip
from . import device as dv
from .band_solver import border_reach, direct_band_solver
from .banded import BandedNotDecoupled, HostPattern, _symbolic_for, share_analysis
from .bordered import bordered_solver
from .device import DeviceCSR, CSRPattern, _p, stream_ptr, ctx
from .device_mode import gather
from .solver_options import current


class LinkedRefused(NotImplementedError):
    """The linked solver declines this matrix (no inner solver under the policy in force, inner
    factorization failed or ill-conditioned, or a pivot of K <= 0): the caller goes on with its
    other solvers."""


class LinkSplit:
    """The rows of A as band rows and link rows, as index lists (host; device copies on first
    use): ``d_rows`` / ``b_rows`` the caller's row index of every link / band row (ascending),
    ``host`` B's pattern and ``b_src`` the positions of its values in ``A.val``, ``c_src`` /
    ``c_dst`` the positions of D's values and where they go in the row-major n x q array D'
    (column * q + link row), ``dst_row`` the row map of ``ipx_link_spmm``."""

    def __init__(self, shape, d_rows, b_rows, host, b_src, c_src, c_dst):
        self.m, self.n = shape
        self.d_rows, self.b_rows, self.q, self.m_b = d_rows, b_rows, len(d_rows), len(b_rows)
        self.host, self.b_src, self.c_src, self.c_dst = host, b_src, c_src, c_dst
        self.dst_row = np.empty(self.m, dtype=np.int64)
        self.dst_row[b_rows] = np.arange(self.m_b)
        self.dst_row[d_rows] = self.m_b + np.arange(self.q)
        self._dev = None

    @property
    def k(self):
        """half bandwidth of B B' (after B's own reordering)"""
        return _symbolic_for(self.host).k

    def on_device(self):
        """(B's CSRPattern carrying the symbolic analysis made on the host, then b_src, c_src,
        c_dst, b_rows, d_rows, dst_row as device tensors)"""
        if self._dev is None:
            dev = ctx().device
            _symbolic_for(self.host)
            pat = share_analysis(self.host, CSRPattern(self.host.indptr_h, self.host.indices_h,
                                                       self.host.shape))
            to = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, dtype=t)).to(dev)
            assert len(self.c_dst) == 0 or (0 <= self.c_dst.min()
                                            and self.c_dst.max() < self.n * self.q)
            assert np.array_equal(np.sort(self.dst_row), np.arange(self.m))
            i32 = np.int32
            self._dev = (pat, to(self.b_src, i32), to(self.c_src, i32), to(self.c_dst, np.int64),
                         to(self.b_rows, i32), to(self.d_rows, i32), to(self.dst_row, i32))
        return self._dev


def split_rows(pattern, rows):
    """``LinkSplit`` with the given link rows (ascending), whatever they look like; None when no
    band row is left."""
    m, n = pattern.shape
    d_rows = np.asarray(rows, dtype=np.int64)
    is_link = np.zeros(m, dtype=bool)
    is_link[d_rows] = True
    b_rows = np.flatnonzero(~is_link)
    if len(b_rows) == 0 or len(d_rows) == 0:
        return None
    counts = np.diff(pattern.indptr_h).astype(np.int64)
    entry_row = np.repeat(np.arange(m, dtype=np.int64), counts)
    entry_link = is_link[entry_row]
    b_src = np.flatnonzero(~entry_link)
    host = HostPattern(np.concatenate(([0], np.cumsum(counts[b_rows]))), pattern.indices_h[b_src],
                       (len(b_rows), n))
    c_src = np.flatnonzero(entry_link)
    local = np.searchsorted(d_rows, entry_row[c_src])
    c_dst = pattern.indices_h[c_src].astype(np.int64) * len(d_rows) + local
    return LinkSplit((m, n), d_rows, b_rows, host, b_src, c_src, c_dst)


def link_split(pattern, reach, limit, border=0):
    """The split of a pattern into band rows and at most ``limit`` link rows, or None.  Two rows
    are coupled when they share a column; a coupled pair further apart than ``reach`` in the
    natural row order is a long edge; the link rows are a vertex cover of the long edges, chosen
    greedily (the row with the most long edges, the lowest index on ties; after every choice the
    distances are those among the rows still present).  What is left has ``B B'`` of half
    bandwidth <= reach in the natural order.  None: a plain band (no long edge),
    long edges left after ``limit`` rows, or no band row left.  A column with more than
    ``reach + 1 + limit`` entries is a clique no cover of that size breaks: None at once -- unless
    up to ``border`` of them may stay in B as border columns (bordered.py), which are then left
    out of the count.  Host, numpy, once per (pattern, reach, limit, border)."""
    cache = pattern.__dict__.setdefault("_ipx_link_split", {})
    key = (int(reach), int(limit), int(border))
    if key not in cache:
        rows = _link_rows(pattern, *key)
        cache[key] = None if rows is None else split_rows(pattern, rows)
    return cache[key]


def _link_rows(pattern, reach, limit, border):
    m, n = pattern.shape
    if limit < 1 or m < 2 or pattern.nnz == 0:
        return None
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(pattern.indptr_h))
    cols = pattern.indices_h.astype(np.int64)
    per_col = np.bincount(cols, minlength=n)
    dense = per_col > reach + 1 + limit
    if dense.any():
        if np.count_nonzero(dense) > border:
            return None
        keep = ~dense[cols]
        rows, cols = rows[keep], cols[keep]
    # entries by (column, row); a row r sits at r + reach inside its column's key range, so the
    # window r - reach .. r + reach never leaves the range
    width = m + 2 * reach + 1
    order = np.lexsort((rows, cols))
    rows, cols = rows[order], cols[order]
    # distances are taken among the rows still present (a removed row no longer separates its
    # neighbours): ``rows`` holds ranks, ``orig`` the caller's index of every rank
    orig = np.arange(m, dtype=np.int64)
    chosen = []
    while True:
        keys = cols * width + rows + reach
        lo = np.searchsorted(keys, keys - reach, side="left")
        hi = np.searchsorted(keys, keys + reach, side="right")
        far = np.bincount(cols, minlength=n)[cols] - (hi - lo)      # per entry: rows out of reach
        count = np.bincount(rows, weights=far, minlength=len(orig))
        if not count.any():
            break
        if len(chosen) == limit:
            return None
        r = int(np.argmax(count))
        chosen.append(int(orig[r]))
        orig = np.delete(orig, r)
        keep = rows != r
        rows, cols = rows[keep], cols[keep]
        rows = rows - (rows > r)
    if not chosen or len(chosen) == m:
        return None
    return np.sort(np.asarray(chosen, dtype=np.int64))


def _inner_solver(B):
    """The solver of B B' under the policy in force: the bordered solver when border columns are
    allowed and B is such a matrix, else ``band_solver.direct_band_solver``'s."""
    try:
        inner = bordered_solver(B)
        if inner is None:
            inner = direct_band_solver(B)
        if inner is None:
            raise LinkedRefused("linked solver: B B' has half bandwidth %d, past the direct "
                                "solvers under the policy %r"
                                % (_symbolic_for(B.pattern).k, current().wide_band))
    except (np.linalg.LinAlgError, BandedNotDecoupled) as exc:
        raise LinkedRefused("linked solver: the factorization of B B' failed (%s)" % exc)
    if getattr(inner, "ill_conditioned", False):
        raise LinkedRefused("linked solver: B B' is numerically rank deficient")
    return inner


class LinkedRowsNormalSolver:
    """(A A')^-1 = block Cholesky on a direct (B B')^-1; ``inner`` is that solver.

    Storage: one tensor, [D' | G | Y | K | L | info | Gram partials | t partials | w_B].  D' is
    the dense n x q transpose of the link rows: 8 n q bytes (256 MB at n = 1e6, q = 32) that stay
    allocated with the solver, as do G and Y (8 m q bytes each)."""

    perm = None        # rows come and go in the caller's order

    def __init__(self, A, split):
        lib = _hip.load()
        self.A = A
        self.m, self.n, self.q, self.m_b = m, n, q, mB = split.m, split.n, split.q, split.m_b
        pat, b_src, c_src, c_dst, self._b_rows, self._d_rows, dst_row = split.on_device()
        self.inner = _inner_solver(DeviceCSR(pat, gather(A.val, b_src)))
        G = self.groups = int(lib.ipx_border_groups(m))
        sizes = (n * q, m * q, m * q, q * q, q * q, 2, G * q * q, G * q, m)
        self.ws = torch.zeros(int(sum(sizes)), dtype=torch.float64, device=ctx().device)
        self.Dt, self.G, self.Y, self.K, self.L, self.info, self._gpart, self._tpart, self._wb = \
            torch.split(self.ws, list(sizes))
        _hip.call("ipx_border_scatter", n, q, c_src.numel(), _p(A.val), _p(c_src), _p(c_dst),
                  _p(self.Dt), stream_ptr())
        p = A.pattern
        _hip.call("ipx_link_spmm", m, n, q, _p(p.indptr), _p(p.indices), _p(A.val), _p(self.Dt),
                  _p(dst_row), _p(self.G), stream_ptr())
        for j in range(q):                      # Y = S_B^-1 E, a column per inner solve; the q
            yj = self.inner.solve(dv._wrap(self.G[j * m:j * m + mB]))     # rows below stay zero
            self.Y[j * m:j * m + mB].copy_(yj.t)
        _hip.call("ipx_border_gram", m, q, _p(self.G), _p(self.Y), _p(self._gpart), stream_ptr())
        _hip.call("ipx_link_chol", m, q, _p(self.G), _p(self._gpart), _p(self.K), _p(self.L),
                  _p(self.info), stream_ptr())
        bits, worst = dv.read_doubles(self.info, 2)          # the one blocking read
        self.flag_bits, self.cancellation = int(bits), float(worst)
        if self.flag_bits & 4:
            raise LinkedRefused("linked solver: the Schur complement of the link rows has a pivot "
                                "<= 0 (max F_jj / K_jj = %.3g)" % self.cancellation)
        self.ill_conditioned = bool(self.flag_bits & 1)
        self.stats = {"solves": 0, "inner_solves": q}

    def solve(self, w):
        """v = (A A')^-1 w, in the caller's row order."""
        m, q = self.m, self.q
        w_b = self._wb[:self.m_b]                            # (the q entries past it stay zero)
        gather(w.t, self._b_rows, out=w_b)
        u = self.inner.solve(dv._wrap(w_b))
        _hip.call("ipx_border_tdot", m, q, _p(self.Y), _p(self._wb), _p(self._tpart), stream_ptr())
        v = dv._empty(m)
        _hip.call("ipx_link_apply", m, q, _p(self.Y), _p(self.L), _p(self._tpart), _p(u.t),
                  _p(w.t), _p(self._b_rows), _p(self._d_rows), _p(v), stream_ptr())
        self.stats["solves"] += 1
        self.stats["inner_solves"] += 1
        return dv._wrap(v)


def _link_split_for(pattern):
    """The link split of a pattern under the options in force, or None (also: option off)."""
    limit = current().link_rows
    if limit < 1:
        return None
    return link_split(pattern, border_reach(), limit, current().border_columns)


def link_solver(A):
    """``LinkedRowsNormalSolver`` for a sparse A when the option is on, the split applies and the
    solver neither refuses nor flags the Schur complement of the link rows as numerically
    singular (``ill_conditioned``: the caller's other choices have their own exits for such a
    matrix); else None."""
    split = _link_split_for(A.pattern) if isinstance(A, DeviceCSR) else None
    if split is None:
        return None
    try:
        solver = LinkedRowsNormalSolver(A, split)
    except LinkedRefused:
        return None
    return None if solver.ill_conditioned else solver
