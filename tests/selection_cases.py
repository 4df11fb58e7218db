"""The catalog of tests/test_gpu_solver_selection.py and tests/test_solver_selection_host.py (no
GPU needed here): small matrices that between them reach every exit of the selection of the
``(A A')^-1`` solver (the rule table), each run under the 12 combinations of
``OPTIONS``.  scripts/record_solver_selection.py recorded what the selection did with them in
tests/golden/solver_selection.json; the tests compare against that file.

A case is ``name -> (builder, max_rows)``: the builder returns a scipy CSR matrix (a numpy array
for the dense case), seeded by the case alone; ``max_rows`` (None: unchanged) is the value
``DenseNormalSolver.MAX_ROWS_FROM_SPARSE`` is patched to, which reaches the exits of m > 16384
with matrices of a few hundred rows (tests/test_gpu_e2e.py does the same).
"""
import itertools

import numpy as np
import scipy.sparse as sps

import blocktri_cases as bc
import blockwide_cases as bw
import bordered_cases as bd
import link_cases as lk
import problems

POLICIES = ("iterative", "block-tridiagonal", "block-tridiagonal-wide")
# (wide_band, border_columns, link_rows)
OPTIONS = tuple(itertools.product(POLICIES, (0, 4), (0, 4)))

# The coupled band: half bandwidth 6, chunks that do not decouple (the matrix of
# test_coupled_wide_band_takes_the_iterative_solver in tests/test_gpu_qp.py, which uses 20000 rows).
# The banded kernels take the partitioned path with its decoupling test only past 2048 rows
# (csrc/banded.hip WIDE_MIN_ROWS): 2049 is the smallest m at which BandedNotDecoupled is raised.
COUPLED_M = 2049
# general rows of the interleaved barrier matrix: 3 m + 4 rows in all, past 2048
INTERLEAVED_M = 700
# ``link_row_nearly_in_the_band``: K / F = 2^(-2 * 19 - 11) = 2^-49, below the 2^-43 at which a pivot
# counts as lost and above the rounding of K that makes it non-positive (on an MI355X the solver
# reports ``ill_conditioned`` for exponents 17 ... 21, a clean factorization up to 16 and refuses a
# pivot <= 0 from 22 on)
ILL_LINK_EXPONENT = 19


def option_id(options):
    return "%s-b%d-l%d" % options


def _sorted(A):
    A = sps.csr_matrix(A)
    A.sort_indices()
    return A


def moving_average_rows(m, k, eps, rng):
    """``_moving_average_rows`` of tests/test_gpu_qp.py: k + 1 nearly equal weights on columns
    i .. i + k plus ``eps`` on a private column; the inverse of A A' decays slowly."""
    cols = (np.arange(m)[:, None] + np.arange(k + 1)[None, :]).ravel()
    rows = np.repeat(np.arange(m), k + 1)
    vals = (1.0 + 0.01 * rng.standard_normal((m, k + 1))).ravel()
    return sps.csr_matrix((np.concatenate((vals, np.full(m, eps))),
                           (np.concatenate((rows, np.arange(m))),
                            np.concatenate((cols, m + k + np.arange(m))))), shape=(m, 2 * m + k))


def barrier_jacobian(J, rng, slack_min=1, slack_max=8, general_slacks=True):
    """The augmented Jacobian of a barrier problem with a box on every variable: general rows
    ``[J | S_c]`` over the bound rows ``-e_j' + s_lb``, ``+e_j' + s_ub`` (integer slacks in
    slack_min ... slack_max).  ``general_slacks=False``: the general rows are J alone (equality
    rows, or rows that bring a private column along)."""
    J = sps.csr_matrix(J)
    m, n = J.shape
    I = sps.eye(n, format="csr")
    s = rng.integers(slack_min, slack_max + 1, m + 2 * n).astype(np.float64)
    return _sorted(sps.bmat([[J, sps.diags(s[:m]) if general_slacks else None, None, None],
                             [-I, None, sps.diags(s[m:m + n]), None],
                             [I, None, None, sps.diags(s[m + n:])]], format="csr"))


def interleaved_barrier(m, eps, rng, slack=64.0):
    """A barrier Jacobian whose NATURAL row order is banded: general row i (three nearly equal
    weights on variables i .. i + 2, ``eps`` on a slack of its own) is followed by the two bound
    rows of variable i.  A A' has half bandwidth 8 (general row i and the upper bound of variable
    i + 2) and, for small eps, a slowly decaying inverse; the general rows alone have half
    bandwidth 2.  Past 2048 rows the banded solver refuses the whole matrix and the box-Schur
    elimination is reached by its second entry."""
    n = m + 2
    rows, cols, vals = [], [], []
    col_slack = n                       # slacks: one per row, after the variables
    r = 0
    w = 1.0 + 0.01 * rng.standard_normal((m, 3))

    def bound_rows(j, r):
        for sign in (-1.0, 1.0):
            rows.extend((r, r))
            cols.extend((j, col_slack + r))
            vals.extend((sign, slack))
            r += 1
        return r

    for i in range(m):
        rows.extend((r,) * 4)
        cols.extend((i, i + 1, i + 2, col_slack + r))
        vals.extend((w[i, 0], w[i, 1], w[i, 2], eps))
        r += 1
        r = bound_rows(i, r)
    for j in (m, m + 1):
        r = bound_rows(j, r)
    return _sorted(sps.csr_matrix((vals, (rows, cols)), shape=(r, n + r)))


def mixed_banded_rows(n=400, m=40):
    """The augmented Jacobian of tests/mixed_banded.py at its starting point: even rows are
    equalities, odd rows inequalities with a slack each, stacked [equalities; inequalities] as the
    canonical form does -- banded only after a reordering of the rows."""
    from ipsolver.synthetic import CenteredBandedNLP
    prob = CenteredBandedNLP(n, m, bw=15, seed=0, eps=1.0)
    J = prob.constr_jac(prob.x0)
    eq, ineq = np.arange(0, m, 2), np.arange(1, m, 2)
    return _sorted(sps.bmat([[J[eq], None], [J[ineq], sps.identity(len(ineq))]], format="csr"))


def _rng(*seed):
    return np.random.default_rng([91] + list(seed))


def _box_coupled_band():
    """Bound rows with large slacks over the coupled band: the Schur complement of the general
    rows stays such a band."""
    J = moving_average_rows(COUPLED_M, 6, 0.1, np.random.default_rng(6))
    return barrier_jacobian(J, _rng(10), 32, 64, general_slacks=False)


def _sparse_barrier():
    p = problems.SparseBarrierQP(n=120, m=80)
    return barrier_jacobian(p.J, _rng(7))


def _bordered(k, m=257, p=2, lim=bd.LIM_BAND):
    rng = _rng(8, k, m, p)
    return bd.bordered(rng, bc.band_rows(rng, m, k, lim=lim), p, 1.0, lim)[0]


def _linked(k, mB=120, q=2):
    return lk.build(k, mB, q, 1.0, False, "middle")[0]


def link_row_nearly_in_the_band(exponent=ILL_LINK_EXPONENT, mB=300, k=4):
    """One link row that is an integer combination of three band rows far apart (entries <= 8)
    but for 2^-exponent on a column of its own: the Schur complement of the link row is
    K = 2^(-2 exponent) exactly, F = D D' is about 2^11, so the pivot of K is positive and below
    2^-43 F -- the linked solver is built and reports ``ill_conditioned``, which ``link_solver``
    declines.  Returns (A, link rows)."""
    rng = _rng(21, mB, k)
    base = bc.band_rows(rng, mB, k, lim=2 ** 3)
    comb = np.zeros(mB)
    comb[[10, mB // 2, mB - 10]] = (1.0, -2.0, 1.0)
    D = np.concatenate((comb @ base.toarray(), [2.0 ** -exponent]))
    base = sps.hstack((base, sps.csr_matrix((mB, 1))), format="csr")
    at = mB // 2
    A = sps.vstack((base[:at], sps.csr_matrix(D), base[at:]), format="csr")
    A.eliminate_zeros()
    return _sorted(A), np.array([at])


def _linked_over_bordered():
    rng = _rng(9)
    base = bd.bordered(rng, bc.band_rows(rng, 120, 4, lim=2 ** 4), 2, 1.0, 2 ** 4)[0]
    return lk.linked(rng, base, 2, 1.0, 2 ** 4, "bottom")[0]


CASES = {
    # ---- ends before any pattern analysis
    "dense": (lambda: _rng(0).standard_normal((5, 12)), None),
    "no-rows": (lambda: sps.csr_matrix((0, 10)), None),
    # ---- the banded solver: natural order, and only after a reordering of the rows
    "band-k1": (lambda: bc.band_rows(_rng(1), 60, 1, lim=2 ** 4), None),
    "band-k8": (lambda: bc.band_rows(_rng(2), 70, 8, lim=2 ** 4), None),
    "band-reordered": (lambda: _sorted(bc.band_rows(_rng(3), 61, 2, lim=2 ** 4)[
        np.concatenate((np.arange(0, 61, 2), np.arange(1, 61, 2)))]), None),
    "mixed-banded": (mixed_banded_rows, None),
    # ---- the box-Schur elimination over a banded Schur complement, by both entries
    "box-band": (lambda: barrier_jacobian(bc.band_rows(_rng(4), 40, 2, lim=2 ** 6), _rng(5)), None),
    "box-interleaved-coupled": (lambda: interleaved_barrier(INTERLEAVED_M, 0.02, _rng(6)), None),
    # ---- BandedNotDecoupled and what follows it
    "coupled-band": (lambda: moving_average_rows(COUPLED_M, 6, 0.1, np.random.default_rng(6)),
                     None),
    "coupled-band-past-dense": (
        lambda: moving_average_rows(COUPLED_M, 6, 0.1, np.random.default_rng(6)), 0),
    "box-coupled-band": (_box_coupled_band, None),
    "box-coupled-band-past-dense": (_box_coupled_band, 0),
    # ---- half bandwidths 9 .. 64 and 65 .. 256
    "ocp-k11": (lambda: bc.ocp_rows(6, 2, 30, _rng(11)), None),
    "ocp-k11-past-dense": (lambda: bc.ocp_rows(6, 2, 30, _rng(11)), 0),
    "band-k64": (lambda: bc.band_rows(_rng(12), 150, 64, lim=2 ** 4), None),
    "moving-average-k9": (lambda: bc.moving_average(90, 9, 64, 1), None),
    "identical-rows-k9": (lambda: bc.identical_rows(_rng(13)), None),
    "band-k65": (lambda: bw.build(65, "selection", 140, False, False)[0], None),
    "band-k65-past-dense": (lambda: bw.build(65, "selection", 140, False, False)[0], 0),
    "band-k256": (lambda: bw.build(256, "selection", 300, False, False)[0], None),
    "band-k257-past-dense": (lambda: bc.band_rows(_rng(14), 300, 257, lim=2 ** 4), 0),
    # ---- (W2): bound rows over general rows with such a band
    "box-ocp-k11": (lambda: barrier_jacobian(bc.ocp_rows(6, 2, 12, _rng(15)), _rng(16)), None),
    "box-band-k65": (lambda: barrier_jacobian(bc.band_rows(_rng(17), 90, 65, lim=2 ** 4),
                                              _rng(18)), None),
    # ---- the box-Schur elimination of any sparsity: dense and iterative Schur solve
    "sparse-barrier": (_sparse_barrier, None),
    "sparse-barrier-dense-schur": (_sparse_barrier, 100),
    "sparse-barrier-past-dense": (_sparse_barrier, 0),
    # ---- border columns: (D1) with each inner solver, (D2), refusals, too many columns
    "bordered-k4": (lambda: _bordered(4), None),
    "bordered-k9": (lambda: _bordered(9), None),
    "bordered-k65": (lambda: _bordered(65, m=300, lim=2 ** 4), None),
    "bordered-5-columns": (lambda: _bordered(4, m=120, p=5), None),
    "box-bordered-k4": (lambda: barrier_jacobian(_bordered(4, m=90), _rng(19)), None),
    "box-bordered-k4-past-dense": (lambda: barrier_jacobian(_bordered(4, m=90), _rng(19)), 0),
    "bordered-huge-growth": (lambda: bd.huge_growth_case()[0], None),
    "bordered-identical-rows": (lambda: bd.identical_rows_case()[0], None),
    "bordered-border-only-row": (lambda: bd.border_only_row_case()[0], None),
    # ---- link rows: (L1) with each inner solver, (L2), declined and refused
    "linked-k4": (lambda: _linked(4), None),
    "linked-k9": (lambda: _linked(9, mB=300), None),
    "linked-over-bordered": (_linked_over_bordered, None),
    "box-linked-k4": (lambda: barrier_jacobian(_linked(4, mB=60), _rng(20)), None),
    "box-linked-k4-past-dense": (lambda: barrier_jacobian(_linked(4, mB=60), _rng(20)), 0),
    "linked-ill-conditioned": (lambda: link_row_nearly_in_the_band()[0], None),
    "linked-nearly-dependent": (lambda: lk.nearly_dependent_case()[0], None),
    "linked-dependent": (lambda: lk.nearly_dependent_case(noise=False)[0], None),
    "linked-identical-link-rows": (lambda: lk.identical_link_rows_case()[0], None),
    "linked-identical-band-rows": (lambda: lk.identical_band_rows_case()[0], None),
}


def build(name):
    """(matrix, max_rows) of a case."""
    builder, max_rows = CASES[name]
    A = builder()
    return (A if isinstance(A, np.ndarray) else _sorted(A)), max_rows
