"""``(A A')^-1`` for a sparse A that is banded / block tridiagonal in ``A A'`` but for a few dense
columns (csrc/bordered.hip): staged problems with global variables -- a free final time, model
parameters, a design variable shared by all stages.

``A = [B | C]`` with C the p dense columns: ``A A' = B B' + C C'``, and by the Woodbury identity

    (S_B + C C')^-1 w = u - Y K^-1 Y' w,   u = S_B^-1 w,   Y = S_B^-1 C,   K = I_p + C' Y,

one solve with the direct factorization of ``S_B = B B'`` (``BandedNormalSolver``,
``BlockTridiagonalNormalSolver`` or its wide form, unchanged) plus O(m p) work.  Opt-in:
``projector.border_columns(limit)``, ``options={"border_columns": limit}``.

Error growth.  ``u - Y z`` cancels when ``C C'`` dominates ``S_B``: the backward error is
``eta ~ c kappa(S_B) kappa_2(K) u``, and since ``K >= I``,
``kappa_2(K) <= lambda_max(K) <= trace(K)`` -- a bound the solver holds anyway (``growth``).
Past ``GROWTH_REFINE`` every solve adds one step of residual refinement on the full system;
past ``GROWTH_MAX`` the solver refuses (``BorderedRefused``) and selection goes on with what it
picks without the option.
"""
import numpy as np
import torch

from . import _hip
from . import device as dv
from .band_solver import border_reach, direct_band_solver
from .banded import BandedNotDecoupled, HostPattern, _symbolic_for, share_analysis  # noqa: F401
from .device import DVec, DeviceCSR, CSRPattern, _p, stream_ptr, ctx
from .device_mode import gather
from .solver_options import current

# eta ~ c kappa_B kappa(K) u with c of order 1 and the projector's orth_tol = 1e-12 ~ 2^13 u:
# up to trace(K) = 2^10 a well-conditioned S_B (kappa_B <= 8) stays below orth_tol without help;
# one refinement step squares the relative error (kappa_B trace(K) u)^2 / u, which is still
# below orth_tol up to trace(K) = 2^26 -- where half of fp64 is gone before the step.
GROWTH_REFINE = 2.0 ** 10
GROWTH_MAX = 2.0 ** 26


class BorderedRefused(NotImplementedError):
    """The bordered solver declines this matrix (inner factorization failed or ill-conditioned,
    or trace(K) past GROWTH_MAX): the caller goes on with its other solvers."""


class BorderSplit:
    """``A = [B | C]`` as index lists into A's values (host; device copies on first use):
    ``cols`` the border columns (ascending), ``b_src`` the positions of B's values, ``c_src`` /
    ``c_dst`` the positions of C's and where they go in the column-major m x p array."""

    def __init__(self, cols, host, b_src, c_src, c_dst):
        self.cols, self.p = cols, len(cols)
        self.host, self.b_src, self.c_src, self.c_dst = host, b_src, c_src, c_dst
        self.m = host.shape[0]
        self._dev = None

    @property
    def k(self):
        """half bandwidth of B B' (after B's own reordering)"""
        return _symbolic_for(self.host).k

    def on_device(self):
        """(B's CSRPattern carrying the symbolic analysis made on the host, b_src, c_src,
        c_dst as device tensors)"""
        if self._dev is None:
            dev = ctx().device
            _symbolic_for(self.host)
            pat = share_analysis(self.host, CSRPattern(self.host.indptr_h, self.host.indices_h,
                                                       self.host.shape))
            to = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, dtype=t)).to(dev)
            assert len(self.c_dst) == 0 or (0 <= self.c_dst.min()
                                            and self.c_dst.max() < self.m * self.p)
            self._dev = (pat, to(self.b_src, np.int32), to(self.c_src, np.int32),
                         to(self.c_dst, np.int64))
        return self._dev


def column_spans(pattern):
    """(last row - first row) per column in the natural row order, -1 for an empty column (what
    ``projector.half_bandwidth_of_aat`` takes the maximum of)."""
    m, n = pattern.shape
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(pattern.indptr_h))
    cols = pattern.indices_h
    first, last = np.full(n, m, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    last[cols] = rows
    first[cols[::-1]] = rows[::-1]
    return np.where(last >= 0, last - first, -1), rows


def border_split(pattern, reach, limit):
    """The split of a pattern into a band and at most ``limit`` border columns, or None.  Border
    columns are those whose span exceeds ``reach``; the split applies when there are 1..limit of
    them, every row keeps an entry outside them, and the rest has ``B B'`` of half bandwidth
    <= reach after B's own reordering.  Host, numpy, once per (pattern, reach, limit)."""
    cache = pattern.__dict__.setdefault("_ipx_border_split", {})
    key = (int(reach), int(limit))
    if key not in cache:
        cache[key] = _border_split(pattern, *key)
    return cache[key]


def _border_split(pattern, reach, limit):
    m, n = pattern.shape
    if limit < 1 or m == 0 or pattern.nnz == 0:
        return None
    spans, _ = column_spans(pattern)
    cols = np.flatnonzero(spans > reach)
    if not 1 <= len(cols) <= limit:
        return None
    split = split_columns(pattern, cols)
    if split is None or split.k > reach:
        return None
    return split


def split_columns(pattern, cols):
    """``BorderSplit`` with the given border columns (ascending), whatever their span; None when a
    row has entries in these columns only."""
    m, n = pattern.shape
    cols = np.asarray(cols, dtype=np.int64)
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(pattern.indptr_h))
    is_border = np.zeros(n, dtype=bool)
    is_border[cols] = True
    entry_border = is_border[pattern.indices_h]
    b_src = np.flatnonzero(~entry_border)
    counts = np.bincount(rows[b_src], minlength=m)
    if not np.all(counts > 0):
        return None                                    # a row with border entries only
    host = HostPattern(np.concatenate(([0], np.cumsum(counts))), pattern.indices_h[b_src], (m, n))
    c_src = np.flatnonzero(entry_border)
    local = np.searchsorted(cols, pattern.indices_h[c_src])
    return BorderSplit(cols, host, b_src, c_src, rows[c_src] + m * local.astype(np.int64))


class BorderedNormalSolver:
    """(A A')^-1 = Woodbury on a direct (B B')^-1; ``inner`` is that solver."""

    perm = None        # rows are taken in the caller's order

    def __init__(self, A, split):
        lib = _hip.load()
        self.A = A
        self.m, self.p = m, p = split.m, split.p
        pat, b_src, c_src, c_dst = split.on_device()
        B = DeviceCSR(pat, gather(A.val, b_src))
        try:
            self.inner = direct_band_solver(B, whatever_the_policy=True)
        except (np.linalg.LinAlgError, BandedNotDecoupled) as exc:
            raise BorderedRefused("bordered solver: the factorization of B B' failed (%s)" % exc)
        if getattr(self.inner, "ill_conditioned", False):
            # Woodbury's error carries kappa(B B'); A A' may be fine where B B' is not
            raise BorderedRefused("bordered solver: B B' is numerically rank deficient")
        G = self.groups = int(lib.ipx_border_groups(m))
        # one tensor owns everything: [C | Y | K | L | info | Gram partials | t partials]
        sizes = (m * p, m * p, p * p, p * p, 2, G * p * p, G * p)
        self.ws = torch.zeros(int(sum(sizes)), dtype=torch.float64, device=ctx().device)
        self.C, self.Y, self.K, self.L, self.info, self._gpart, self._tpart = \
            torch.split(self.ws, list(sizes))
        _hip.call("ipx_border_scatter", m, p, c_src.numel(), _p(A.val), _p(c_src), _p(c_dst),
                  _p(self.C), stream_ptr())
        for j in range(p):                      # Y = S_B^-1 C, a column per inner solve
            yj = self.inner.solve(dv._wrap(self.C[j * m:(j + 1) * m]))
            self.Y[j * m:(j + 1) * m].copy_(yj.t)
        _hip.call("ipx_border_gram", m, p, _p(self.C), _p(self.Y), _p(self._gpart), stream_ptr())
        _hip.call("ipx_border_chol", m, p, _p(self._gpart), _p(self.K), _p(self.L),
                  _p(self.info), stream_ptr())
        bits, growth = dv.read_doubles(self.info, 2)         # the one blocking read
        self.flag_bits, self.growth = int(bits), float(growth)
        if self.flag_bits & 4 or not self.growth <= GROWTH_MAX:
            raise BorderedRefused("bordered solver: trace(K) = %.3g (limit %.3g), pivot bits %d"
                                  % (self.growth, GROWTH_MAX, self.flag_bits))
        self.ill_conditioned = bool(self.flag_bits & 1)
        self.refine = self.growth > GROWTH_REFINE
        self.stats = {"solves": 0, "refinements": 0, "inner_solves": p}

    def _solve0(self, w):
        u = self.inner.solve(w)
        _hip.call("ipx_border_tdot", self.m, self.p, _p(self.Y), _p(w.t), _p(self._tpart),
                  stream_ptr())
        _hip.call("ipx_border_apply", self.m, self.p, _p(self.Y), _p(self.L), _p(self._tpart),
                  _p(u.t), _p(u.t), stream_ptr())
        self.stats["inner_solves"] += 1
        return u

    def solve(self, w):
        """v = (A A')^-1 w, in the caller's row order."""
        v = self._solve0(w)
        if self.refine:
            # one step on the full system: r = w - A (A' v), v += solve0(r)
            r = self.A.spmv(self.A.T.dot(v), alpha=-1.0, beta=1.0, yin=w)
            v = v + self._solve0(r)
            self.stats["refinements"] += 1
        self.stats["solves"] += 1
        return v


def _border_split_for(pattern):
    """The border split of a pattern under the options in force, or None (also: option off)."""
    limit = current().border_columns
    if limit < 1:
        return None
    return border_split(pattern, border_reach(), limit)


def bordered_solver(A):
    """``BorderedNormalSolver`` for a sparse A when the option is on, the split applies and the
    solver does not refuse; else None (the caller's other choices)."""
    split = _border_split_for(A.pattern) if isinstance(A, DeviceCSR) else None
    if split is None:
        return None
    try:
        return BorderedNormalSolver(A, split)
    except BorderedRefused:
        return None
