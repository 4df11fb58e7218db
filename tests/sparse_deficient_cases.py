"""Rank-deficient sparse Jacobians for the tests of ``sparse_rank_deficient = "skip-pivots"``
(ipsolver/sparse_deficient.py): builders shared by tests/test_sparse_deficient_host.py,
tests/test_gpu_sparse_deficient.py, tests/test_gpu_sparse_deficient_e2e.py and the fixture's
generator tests/golden/make_golden_sparse_rank_deficient.py.

``G`` is the node-arc incidence matrix of the N x N grid (tests/two_level_cases.py without its
``eps I`` columns): rank m - 1.  The other cases replace or add rows of the full-rank
``grid(N, 0.125) = [G, 2^-3 I]``.  Every matrix is scaled by 2^-10 (exact; the reason is
tests/rank_deficient_cases.py's: the oracle's absolute tol = 1e-15).  All entries are small
integers times a power of two, so ``A_S A_S'`` is exact and tests/normal_ref.py evaluates
residuals exactly.

The duplicate-row cases are FOUND, not listed: ``lds_position_cases`` / ``tiled_position_cases``
search over (row, neighbouring row) pairs until the skipped pivot lands at the wanted places of
the library's elimination order -- the last own row of a front, a leaf and a separator front,
two in one front; positions 15, 16, 63, 64, s - 1 of a tiled leaf front.  Position 0 (the first
own row of a front) is reached by zero rows only: see ``TILED_FIRST``.
"""
import functools

import numpy as np
import scipy.sparse as sps

import sparse_deficient_model as model
import two_level_cases as tc

SCALE = 2.0 ** -10
ORACLE_TOL = 1e-15
EPS_COLUMNS = 0.125
LDS = (12, 32, None)                    # N, LEAF, SMALL_FRONT: every front in LDS
TILED = (16, 128, 32)                   # leaf fronts own 65 ... 128 rows: two tile columns


def _csr(A):
    A = sps.csr_matrix(A)
    A.eliminate_zeros()
    A.sort_indices()
    return A


def pure_g(N):
    edges = 2 * N * (N - 1)
    return _csr(tc.grid(N, EPS_COLUMNS)[:, :edges] * SCALE)


def thinned_g(N=24, removed=0.45, seed=1):
    keep = np.random.default_rng(seed).random(2 * N * (N - 1)) >= removed
    return _csr(tc.flow_matrix(N, EPS_COLUMNS, keep)[:, :int(keep.sum())] * SCALE)


def full_grid(N):
    return _csr(tc.grid(N, EPS_COLUMNS) * SCALE)


def with_rows(A, replaced=(), appended=()):
    """A with row j replaced by the given (1 x n) row for every (j, row) of ``replaced``, and the
    rows of ``appended`` below it."""
    rows = [A[i] for i in range(A.shape[0])]
    for j, row in replaced:
        rows[j] = sps.csr_matrix(row)
    return _csr(sps.vstack(rows + [sps.csr_matrix(r) for r in appended], format="csr"))


def duplicated(N, pairs):
    """grid(N) with row j a copy of row i for every (j, i)."""
    A = full_grid(N)
    return with_rows(A, replaced=[(j, A[i]) for j, i in pairs])


def combination(N=12):
    A = full_grid(N)
    return with_rows(A, replaced=[(40, A[5] + A[6] - 2 * A[17])])


def two_zero_rows(N=12):
    A = full_grid(N)
    zero = sps.csr_matrix((1, A.shape[1]))
    return with_rows(A, replaced=[(7, zero), (100, zero)])


def appended_sum(N=24):
    A = full_grid(N)
    return with_rows(A, appended=[sps.csr_matrix(A.sum(axis=0))])


def _neighbours(j, N):
    """The rows within two grid steps of row j, the nearest first."""
    r, c = divmod(j, N)
    steps = [(0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1),
             (0, 2), (2, 0), (0, -2), (-2, 0)]
    return [(r + dr) * N + c + dc for dr, dc in steps if 0 <= r + dr < N and 0 <= c + dc < N]


def _landing(N, leaf, pairs, A=None):
    """Where the skipped pivots of ``duplicated(N, pairs)`` land by the ORDER alone (of two equal
    rows the later one goes): [(supernode, position inside it, own rows, tree level)].  ``A``:
    another matrix to take the order from (the search's first guess)."""
    sym = model.analysis(duplicated(N, pairs) if A is None else A, leaf)
    pos = np.empty(sym.m, dtype=np.int64)
    pos[sym.perm] = np.arange(sym.m)
    out = []
    for j, i in pairs:
        k = max(pos[i], pos[j])
        sn = int(np.searchsorted(sym.sn_ptr, k, side="right") - 1)
        out.append((sn, int(k - sym.sn_ptr[sn]), int(sym.own[sn]), int(sym.level[sn])))
    return out


def _search(N, leaf, wanted):
    """name -> ((j, i),) for every predicate of ``wanted`` (name -> f(position, s, level)): the
    first pair (rows ascending, partners nearest first) that meets it; names not found are
    missing.  A copied row changes the pattern and with it the order, so every pair is judged by
    the analysis of ITS matrix; the order of the unchanged grid only says which pairs to try."""
    base = full_grid(N)
    pairs = [(j, i) for j in range(N * N) for i in _neighbours(j, N)]
    guess = {pair: _landing(N, leaf, [pair], base)[0] for pair in pairs}
    found = {}
    for name, test in wanted.items():
        for pair in pairs:
            if test(*guess[pair][1:]) and test(*_landing(N, leaf, [pair])[0][1:]):
                found[name] = (pair,)
                break
    return found


@functools.lru_cache(maxsize=None)
def lds_position_cases():
    """name -> pairs, on grid(12) with leaves of 32 rows."""
    N, leaf, _ = LDS
    found = _search(N, leaf, {
        "last-own-row": lambda p, s, lv: p == s - 1 and s > 1,
        "leaf-front": lambda p, s, lv: lv == 0 and 0 < p < s - 1,
        "separator-front": lambda p, s, lv: lv > 0 and 0 < p < s - 1,
    })
    # two skips in one front: a second pair beside the leaf front's, far enough to leave the
    # first where it is
    if "leaf-front" in found:
        first = found["leaf-front"][0]
        near = [(j, i) for j in _neighbours(first[0], N) for i in _neighbours(j, N)[:4]
                if not {i, j} & set(first)]
        for pair in near:
            a, b = _landing(N, leaf, [first, pair])
            if a[0] == b[0] and a[1] != b[1]:
                found["two-in-one-front"] = (first, pair)
                break
    return found


# Position 0 of a front.  Two equal rows have the same neighbours in the graph of A A', so every
# dissection leaves them in the same part and in the end in the same front, where the first is
# kept: no duplicate lands on a front's first own row, and in a front without children nothing
# is eliminated before that row at all.  (Scans over sums of two neighbouring rows found no such
# landing either.)  What does land there is a zero row -- a piece of its own, a front of one own
# row, S_kk = 0: "two-zero-rows" on the LDS path, and the same matrix with EVERY front tiled
# (SMALL_FRONT 0) for position 0 of the tiled path.
TILED_FIRST = (12, 32, 0)               # every front by tiles
TILED_POSITIONS = (0, 15, 16, 63, 64, "last")


@functools.lru_cache(maxsize=None)
def tiled_position_cases():
    """name -> pairs, on grid(16) with leaves of 128 rows: leaf fronts that own more than 64.
    Position 0: the case "tile-0" (see above)."""
    N, leaf, _ = TILED
    wanted = {}
    for p0 in TILED_POSITIONS[1:]:
        if p0 == "last":
            wanted["tile-last"] = lambda p, s, lv: lv == 0 and s > 64 and p == s - 1
        else:
            wanted["tile-%d" % p0] = lambda p, s, lv, p0=p0: lv == 0 and s > 64 and p == p0
    return _search(N, leaf, wanted)


# name -> (builder, LEAF, SMALL_FRONT); every one within the cap of 32 dropped rows
def all_cases():
    out = {
        "G6": (lambda: pure_g(6), 32, None),
        "G12": (lambda: pure_g(12), 32, None),
        "G12-tiled": (lambda: pure_g(12), 32, 32),
        "combination": (combination, 32, None),
        "two-zero-rows": (two_zero_rows, 32, None),
        "appended-sum": (appended_sum, 32, None),
    }
    out["tile-0"] = (two_zero_rows,) + TILED_FIRST[1:]
    for name, pairs in lds_position_cases().items():
        out["lds-" + name] = (functools.partial(duplicated, LDS[0], pairs), LDS[1], LDS[2])
    for name, pairs in tiled_position_cases().items():
        out[name] = (functools.partial(duplicated, TILED[0], pairs), TILED[1], TILED[2])
    return out


@functools.lru_cache(maxsize=None)
def built(name):
    """(A, LEAF, SMALL_FRONT, analysis, model) of a case, once."""
    build, leaf, small = all_cases()[name]
    A = build()
    sym = model.analysis(A, leaf)
    return A, leaf, small, sym, model.SkippingCholesky(A, sym.perm)


def oracle_rank(A):
    """The rank the oracle's SVD exit works with (singular values > tol)."""
    import scipy.linalg
    return int(np.count_nonzero(scipy.linalg.svd(A.toarray(), compute_uv=False) > ORACLE_TOL))


def oracle_svd_operators(A):
    """The oracle's SVD operators (its exit for a singular Jacobian, asked for by name: its sparse
    default, SuperLU on the augmented system, does not always notice a singular matrix)."""
    import oracle
    return oracle.projections(A.toarray(), method="SVDFactorization")


def conditions(A, kept):
    """(sigma_1 / sigma_rank of A, cond of the kept rows A_S)."""
    import scipy.linalg
    s = scipy.linalg.svd(A.toarray(), compute_uv=False)
    rank = int(np.count_nonzero(s > ORACLE_TOL))
    sk = scipy.linalg.svd(A[kept].toarray(), compute_uv=False)
    return float(s[0] / s[rank - 1]), float(sk[0] / sk[-1])


# ---- the end-to-end problems: min 1/2 ||x||^2 + c'x subject to flow balance rows
def flow_qp(A, seed):
    """(c, b) for the rows A: a random c, and b = A x0 (consistent whatever the rank)."""
    n = A.shape[1]
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n), A.dot(rng.standard_normal(n))


E2E_SMALL_SEED = 21


def e2e_small():
    """(A, c, b, independent): the flow QP at N = 12 on pure G (rank m - 1); ``independent``:
    all rows but the last (the incidence matrix of a connected graph without any one of its rows
    has full rank)."""
    A = pure_g(12)
    c, b = flow_qp(A, E2E_SMALL_SEED)
    return A, c, b, np.arange(A.shape[0] - 1)


def kkt_point(A, c, b):
    """The minimiser of 1/2 ||x||^2 + c'x on A x = b for a sparse A of full row rank, by an LU
    factorization of the KKT matrix [[I, A'], [A, 0]] (scipy.sparse.linalg.splu)."""
    import scipy.sparse.linalg
    m, n = A.shape
    K = sps.bmat([[sps.identity(n), A.T], [A, None]], format="csc")
    return scipy.sparse.linalg.splu(K).solve(np.concatenate((-c, b)))[:n]


E2E_LARGE_N = 80
E2E_LARGE_SEED = 22


def e2e_large():
    """(A, c, b, independent): grid(80, 0.125) (6400 rows, m n = 1.2e8 > 2^25) and three appended
    rows -- two duplicates and one three-term combination --, b extended consistently;
    ``independent``: the 6400 rows of the grid."""
    A0 = full_grid(E2E_LARGE_N)
    m = A0.shape[0]
    extra = [A0[1234], A0[4321], A0[100] + A0[101] - 2 * A0[3000]]
    A = with_rows_appended(A0, extra)
    c, b = flow_qp(A, E2E_LARGE_SEED)
    return A, c, b, np.arange(m)


def with_rows_appended(A, rows):
    return _csr(sps.vstack([A] + [sps.csr_matrix(r) for r in rows], format="csr"))
