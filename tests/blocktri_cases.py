"""Matrix generators and the case list of tests/test_gpu_blocktri.py (no GPU needed here).

``band_rows`` and ``moving_average`` restate the generators of tests/test_gpu_normal_solve.py
with the value limit as a parameter; ``ocp_rows`` is the staged pattern of discretised
dynamics.  Every matrix is integer-valued, so ``normal_ref.gram_pow2``, ``residual_exact`` and
``backward_error`` apply unchanged.
"""
import numpy as np
import scipy.sparse as sps

import normal_ref as nr

BLOCK_OF_K = {9: 16, 16: 16, 17: 32, 32: 32, 33: 64, 64: 64}
KS = sorted(BLOCK_OF_K)
EDGE_N = (1, 2, 3, 4, 5, 8, 9)          # one block, the first level, odd / even counts at three levels
EDGE_DELTA = (-1, 0, 1)
TAIL_ROWS = {16: 32, 32: 16, 64: 8}     # ipx_blocktri_levels out[1] (the GPU test checks it)
GRADED_N = 5

# kappa_2 of the diagonally scaled S, checked by tests/test_blocktri_host.py
KAPPA_PLAIN, KAPPA_PRIVATE = 34.0, 4.3


def _csr(vals, rows, cols, shape):
    A = sps.csr_matrix((np.asarray(vals, dtype=np.float64), (rows, cols)), shape=shape)
    A.sort_indices()
    return A


def lim_for(k):
    """Largest |entry| that keeps every entry of S within 26 significant bits (private column
    included): 2^8 up to k = 17, 2^7 past it."""
    return 2 ** 8 if k <= 17 else 2 ** 7


def band_rows(rng, m, k, lim=2 ** 10, private=False):
    """Random integer rows over columns 3i .. 3i + 3k: A A' of half bandwidth min(k, m - 1),
    well conditioned.  ``private``: plus an entry in [2^11, 2^12) on a column of its own."""
    w = 3 * k + 1
    cols = (3 * np.arange(m)[:, None] + np.arange(w)[None, :]).ravel()
    rows, vals, n = np.repeat(np.arange(m), w), nr.int_values(rng, m * w, lim), 3 * m + 3 * k + 1
    if private:
        rows = np.concatenate((rows, np.arange(m)))
        cols = np.concatenate((cols, n + np.arange(m)))
        vals = np.concatenate((vals, rng.integers(2 ** 11, 2 ** 12, m).astype(np.float64)))
        n += m
    return _csr(vals, rows, cols, (m, n))


def moving_average(m, k, W, eps, rng=None, noise=0):
    """Row i: weight W (+ integer noise) on columns i .. i + k and eps on a private column:
    nearly dependent neighbours for eps << W (cond ~ ((k + 1) W / eps)^2), half bandwidth k."""
    vals = np.full((m, k + 1), W, dtype=np.int64)
    if noise:
        vals = vals + rng.integers(-noise, noise + 1, (m, k + 1))
    cols = (np.arange(m)[:, None] + np.arange(k + 1)[None, :]).ravel()
    rows = np.repeat(np.arange(m), k + 1)
    return _csr(np.concatenate((vals.ravel(), np.full(m, eps))),
                np.concatenate((rows, np.arange(m))),
                np.concatenate((cols, m + k + np.arange(m))), (m, 2 * m + k))


def ocp_rows(d, c, stages, rng, lim=2 ** 6):
    """Discretised dynamics: stage t has d states and c controls (columns t (d + c) ..), its d
    constraint rows touch x_t, u_t and one component of x_{t+1}.  J J' is block tridiagonal in
    blocks of d: half bandwidth 2 d - 1.  Integer values of magnitude <= lim."""
    w = d + c
    own = (np.arange(stages)[:, None, None] * w + np.arange(w)[None, None, :]
           + np.zeros((1, d, 1), dtype=np.int64))                     # (stages, d, w)
    nxt = (np.arange(stages)[:, None] + 1) * w + np.arange(d)[None, :]  # (stages, d)
    cols = np.concatenate((own, nxt[:, :, None]), axis=2).ravel()
    rows = np.repeat(np.arange(stages * d), w + 1)
    return _csr(nr.int_values(rng, len(cols), lim), rows, cols, (stages * d, (stages + 1) * w))


def half_bandwidth(S):
    coo = sps.coo_matrix(S)
    return int(np.max(np.abs(coo.row - coo.col))) if coo.nnz else 0


# ---------------------------------------------------------------------------- the case list
def edge_cases(k):
    """(name, m, private, graded) of the solve test for half bandwidth k."""
    b = BLOCK_OF_K[k]
    out = []
    for N in EDGE_N:
        for delta in EDGE_DELTA:
            m = N * b + delta
            if m >= 1:
                out.append(("N%d%+d" % (N, delta), m, False, False))
    out.append(("launched", (2 * TAIL_ROWS[b] + 1) * b, False, False))
    out.append(("graded", GRADED_N * b + 1, False, True))
    out.append(("graded-private", GRADED_N * b + 1, True, True))
    return out


def build(k, name, m, private, graded):
    """(A_int, e, w) of a case: seeded by the case alone."""
    seed = [k, m, int(private), int(graded)]
    rng = np.random.default_rng(seed)
    A = band_rows(rng, m, k, lim=lim_for(k), private=private)
    e = rng.integers(-30, 31, m) if graded else np.zeros(m, np.int64)
    spread = 30 if graded else 4
    w = rng.standard_normal(m) * np.ldexp(1.0, rng.integers(-spread, spread + 1, m))
    return A, e, w


def identical_rows(rng, m=40, k=9, at=16):
    """A band with rows ``at`` and ``at + 1`` identical: sixteen entries +-4, so S[at, at] = 256
    and its square root, the quotient 256 / 16 and the pivot 256 - 16 * 16 = 0 are all exact."""
    A = band_rows(rng, m, k, lim=2 ** 4).tolil()
    cols = list(range(3 * at, 3 * at + 16))
    vals = list(4.0 * rng.choice((-1, 1), 16))
    for r in (at, at + 1):
        A.rows[r], A.data[r] = list(cols), list(vals)
    A = A.tocsr()
    A.sort_indices()
    return A


def staged_problem(d=6, c=2, stages=30, seed=0):
    """The staged test problem of the public call: J (ocp_rows / 64), a feasible point inside
    the box [-2, 2], the target of the quadratic objective."""
    rng = np.random.default_rng(seed)
    J = ocp_rows(d, c, stages, rng) * (1.0 / 64)
    n = J.shape[1]
    x_feas = rng.uniform(-1, 1, n)
    target = rng.uniform(-1, 1, n)
    return J.tocsr(), J @ x_feas, target
