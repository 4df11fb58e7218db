"""The scoped options of the ``(A A')^-1`` solver selection (selection.py), in one record.

``wide_band``: what takes a sparse A whose ``A A'`` is banded past the banded kernels' half
bandwidth -- "iterative" (default): the dense Cholesky while it fits, else the preconditioned CG;
"block-tridiagonal": block cyclic reduction (blocktri.py) up to half bandwidth 64;
"block-tridiagonal-wide": the same, and blocks of 128 / 256 (blockwide.py) for half bandwidths
65 ... 256.

``border_columns``: up to this many columns of a sparse A may be split off as a border when the
rest is banded / block tridiagonal in ``A A'`` (bordered.py).  ``link_rows``: likewise up to this
many rows (linked.py).  0, the default of both: off, every path as without the option.

``iterative_precond``: the preconditioner of every ``IterativeNormalSolver`` (iterative.py) that
is built without an explicit one -- "block" (default), "compact" or "two-level".  It is held
beside the three fields above, which stay the tuple: ``key()`` appends it only when it is not the
default, so the keys of every setting that existed before it are what they were.

``sparse_direct``: "off" (default), or "nested-dissection": a sparse A that no band solver takes
and (without the option) the dense Cholesky or the preconditioned CG would, is factored by the
nested-dissection multifrontal Cholesky (nested.py).  Held and keyed like ``iterative_precond``.

``dense_factorization``: "normal-equations" (default): a dense Jacobian is factored as Gram +
Cholesky (dense.py); "householder-qr": by a blocked Householder QR of ``A'`` on the device
(dense_qr.py), whose operators lose ``cond(A) eps`` instead of ``cond(A)^2 eps``.  It acts on
dense device matrices only -- a sparse Jacobian ignores it.  Held and keyed like
``iterative_precond``.

``rank_deficient``: "host-svd" (default): a Jacobian that a factorization finds numerically rank
deficient takes the reference's exit, LAPACK's SVD on the host (``SVDProjector``); "pivoted-qr":
a dense device Jacobian with ``1 <= m <= n`` is factored by a column-pivoted QR on the device
instead (``DenseCODProjector``, dense_cod.py) -- sparse Jacobians, ``m > n`` and
``method="SVDFactorization"`` keep the host exit.  Held and keyed like ``iterative_precond``.

``sparse_rank_deficient``: "host-svd" (default): a SPARSE Jacobian found rank deficient takes the
host exit above (capped at ``m n <= 2^25`` elements); "skip-pivots": it is factored once more on
the device by the nested-dissection Cholesky in pivot-skipping mode, whatever ``sparse_direct``
says, and the pseudo-inverse operators come from that factorization and a Woodbury correction over
the dropped rows (``SparseDeficientProjector``, sparse_deficient.py) -- more than 32 dropped rows,
a matrix past the nested solver's limits and ``method="SVDFactorization"`` keep the host exit.
Held and keyed like ``iterative_precond``.

Scoped: ``with scoped(wide_band="block-tridiagonal", link_rows=4): ...`` holds any subset for the
duration of the block.  ``current().key()`` is part of the key of every cached factorization: a
new option is a new name here (``NAMES``, ``check``, ``key``) and nowhere else.
"""
import collections
import contextlib

import numpy as np

from . import _hip

WIDE_BAND_POLICIES = ("iterative", "block-tridiagonal", "block-tridiagonal-wide")
ITERATIVE_PRECONDS = ("block", "compact", "two-level")
SPARSE_DIRECT = ("off", "nested-dissection")
DENSE_FACTORIZATIONS = ("normal-equations", "householder-qr")
RANK_DEFICIENT = ("host-svd", "pivoted-qr")
SPARSE_RANK_DEFICIENT = ("host-svd", "skip-pivots")
NAMES = ("wide_band", "border_columns", "link_rows", "iterative_precond", "sparse_direct",
         "dense_factorization", "sparse_rank_deficient", "rank_deficient")
# the options held beside the tuple: name -> allowed values, the first the default
_BESIDE = {"iterative_precond": ITERATIVE_PRECONDS, "sparse_direct": SPARSE_DIRECT,
           "dense_factorization": DENSE_FACTORIZATIONS, "rank_deficient": RANK_DEFICIENT,
           "sparse_rank_deficient": SPARSE_RANK_DEFICIENT}


class Options(collections.namedtuple("Options", "wide_band border_columns link_rows")):
    iterative_precond = ITERATIVE_PRECONDS[0]      # (attributes beside the tuple's fields)
    sparse_direct = SPARSE_DIRECT[0]
    dense_factorization = DENSE_FACTORIZATIONS[0]
    rank_deficient = RANK_DEFICIENT[0]
    sparse_rank_deficient = SPARSE_RANK_DEFICIENT[0]

    def __new__(cls, wide_band, border_columns, link_rows, iterative_precond="block",
                sparse_direct="off", dense_factorization="normal-equations",
                rank_deficient="host-svd", sparse_rank_deficient="host-svd"):
        self = super().__new__(cls, wide_band, border_columns, link_rows)
        self.iterative_precond = iterative_precond
        self.sparse_direct = sparse_direct
        self.dense_factorization = dense_factorization
        self.rank_deficient = rank_deficient
        self.sparse_rank_deficient = sparse_rank_deficient
        return self

    def _replace(self, **changes):
        beside = {name: changes.pop(name, getattr(self, name)) for name in _BESIDE}
        new = super()._replace(**changes)
        for name, value in beside.items():
            setattr(new, name, value)
        return new

    def key(self):
        """What tells two settings apart in a cache key."""
        extra = () if self.iterative_precond == ITERATIVE_PRECONDS[0] else (self.iterative_precond,)
        if self.sparse_direct != SPARSE_DIRECT[0]:
            extra += (self.sparse_direct,)
        if self.dense_factorization != DENSE_FACTORIZATIONS[0]:
            extra += (self.dense_factorization,)
        if self.rank_deficient != RANK_DEFICIENT[0]:
            extra += (self.rank_deficient,)
        if self.sparse_rank_deficient != SPARSE_RANK_DEFICIENT[0]:
            extra += (self.sparse_rank_deficient,)
        return tuple(self) + extra


_current = [Options("iterative", 0, 0)]


def current():
    return _current[0]


def check(name, value):
    """``value`` as option ``name`` holds it, or ValueError."""
    if name == "wide_band":
        if value not in WIDE_BAND_POLICIES:
            raise ValueError("wide_band must be one of %s, not %r"
                             % (", ".join(repr(p) for p in WIDE_BAND_POLICIES), value))
        return value
    if name in _BESIDE:
        if value not in _BESIDE[name]:
            raise ValueError("%s must be one of %s, not %r"
                             % (name, ", ".join(repr(p) for p in _BESIDE[name]), value))
        return value
    if name not in Options._fields:
        raise ValueError("unknown solver option %r" % (name,))
    most = _hip.load().ipx_border_pmax()
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) \
            or not 0 <= value <= most:
        raise ValueError("%s must be an integer in 0 ... %d, not %r" % (name, most, value))
    return int(value)


@contextlib.contextmanager
def scoped(**changes):
    """Hold the given options for the duration of the block (restored on any exit)."""
    previous = _current[0]
    _current[0] = previous._replace(**{name: check(name, v) for name, v in changes.items()})
    try:
        yield
    finally:
        _current[0] = previous


def pop_from(options):
    """The solver options of a user's ``options`` dict, checked and taken out of it (an option
    that is not given: the value in force), as the keywords of ``scoped``."""
    held = {name: check(name, options.pop(name, getattr(current(), name)))
            for name in NAMES[:4]}
    # (``sparse_direct``, ``dense_factorization``, ``sparse_rank_deficient`` and
    # ``rank_deficient`` only when given: without it ``scoped`` leaves the value in force as it
    # is, and the record of a call that does not use it reads as before the option)
    for name in NAMES[4:]:
        if name in options:
            held[name] = check(name, options.pop(name))
    return held


def _wrappers(name):
    def hold(value):
        return scoped(**{name: value})

    def get():
        return getattr(current(), name)

    def check_one(value):
        return check(name, value)
    hold.__doc__ = "Hold ``%s`` for the duration of the block (restored on any exit)." % name
    return hold, get, check_one


# the names callers have used since each option was added
wide_band, wide_band_policy, check_wide_band = _wrappers("wide_band")
border_columns, border_columns_limit, check_border_columns = _wrappers("border_columns")
link_rows, link_rows_limit, check_link_rows = _wrappers("link_rows")
iterative_precond, iterative_precond_choice, check_iterative_precond = \
    _wrappers("iterative_precond")
sparse_direct, sparse_direct_choice, check_sparse_direct = _wrappers("sparse_direct")
dense_factorization, dense_factorization_choice, check_dense_factorization = \
    _wrappers("dense_factorization")
rank_deficient, rank_deficient_choice, check_rank_deficient = _wrappers("rank_deficient")
sparse_rank_deficient, sparse_rank_deficient_choice, check_sparse_rank_deficient = \
    _wrappers("sparse_rank_deficient")
