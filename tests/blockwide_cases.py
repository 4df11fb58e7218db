"""The case list of tests/test_gpu_blockwide.py (no GPU needed here): the generators are those of
tests/blocktri_cases.py, at half bandwidths 65 ... 256 (blocks of 128 and 256).

Matrices: ``band_rows(rng, m, k, lim=2**7, private=...)``.  With |entry| <= 2^7 an entry of S
is a sum of at most 3 k + 1 products, |S_ij| <= (3 k + 1) 2^14 + 2^24 < 2^26 for k <= 256 (the
2^24: the square of the private entry), so ``normal_ref.residual_exact``'s 26-bit condition holds.
"""
import numpy as np

import blocktri_cases as bc

BLOCK_OF_K = {65: 128, 128: 128, 129: 256, 256: 256}
KS = sorted(BLOCK_OF_K)
EDGE_N = (1, 2, 3, 5)                   # one block, the first level, odd counts at two levels
EDGE_DELTA = (-1, 0, 1)
DEEP_N = 9                              # + 1 row: four levels of their own
GRADED_N = 3
LIM = 2 ** 7

# kappa_2 of the diagonally scaled S over the cases below, checked (and printed) by
# tests/test_blockwide_host.py: largest found 32.9 (plain, k = 129), 5.25 (private, k = 256)
KAPPA_PLAIN, KAPPA_PRIVATE = 34.0, 5.5


def edge_cases(k):
    """(name, m, private, graded) of the solve test for half bandwidth k.  There is no
    one-workgroup tail (ipx_blockwide_levels: out[1] = 1), so every level of every case is a
    launch of its own and no case is needed for "the first level beyond the tail"."""
    b = BLOCK_OF_K[k]
    out = []
    for N in EDGE_N:
        for delta in EDGE_DELTA:
            out.append(("N%d%+d" % (N, delta), N * b + delta, False, False))
    out.append(("N%d+1" % DEEP_N, DEEP_N * b + 1, False, False))
    out.append(("graded", GRADED_N * b + 1, False, True))
    out.append(("graded-private", GRADED_N * b + 1, True, True))
    return out


def levels(m, b):
    """1 + ceil(log2 N): what ipx_blockwide_levels reports in out[0]."""
    n, L = -(-m // b), 1
    while n > 1:
        n, L = (n + 1) // 2, L + 1
    return L


def build(k, name, m, private, graded):
    """(A_int, e, w) of a case: seeded by the case alone."""
    rng = np.random.default_rng([k, m, int(private), int(graded)])
    A = bc.band_rows(rng, m, k, lim=LIM, private=private)
    e = rng.integers(-30, 31, m) if graded else np.zeros(m, np.int64)
    spread = 30 if graded else 4
    w = rng.standard_normal(m) * np.ldexp(1.0, rng.integers(-spread, spread + 1, m))
    return A, e, w
