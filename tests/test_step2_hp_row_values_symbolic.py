"""The symbolic side of k_cg_step2_hp's index-free tiles (ipsolver.cg_fused), numpy in and numpy
out, no device:

* ``shifted_tiles_np``: which uniform row tiles are shifted-contiguous -- entry k of row i at
  span offset ``col16[s] + i + k`` -- so that the kernel forms their column offsets;
* ``rowmajor_tiles_map_np``: the gather map that stores such tiles' values entry-major
  (``valT[s + k nrows + i] = val[s + i rl + k]``) where their rows hold at most four entries.

The tiles are cut here by hand (whole rows, at most 2 048 entries and 1 024 rows to a tile) and
the offsets are taken against ``max(r0 - hmax, 0)``, as ``compact_columns`` takes them.
"""
import numpy as np
import pytest
import scipy.sparse as sps

from ipsolver import cg_fused

TILE_NNZ, TILE_ROWS = 2048, 1024


def cut(H):
    """(row bounds, entry bounds) of the row tiles: whole rows, greedily."""
    indptr = H.indptr.astype(np.int64)
    rows = [0]
    while rows[-1] < H.shape[0]:
        r0 = rows[-1]
        r1 = r0 + 1
        while (r1 < H.shape[0] and r1 - r0 < TILE_ROWS
               and indptr[r1 + 1] - indptr[r0] <= TILE_NNZ):
            r1 += 1
        rows.append(r1)
    rows = np.array(rows)
    return rows, indptr[rows]


def tables(H):
    """(col16, rowlen, entry bounds, row bounds) as compact_columns makes them."""
    H = H.tocsr()
    H.sort_indices()
    rows, bounds = cut(H)
    lens = np.diff(H.indptr)
    hmax = int(max(np.max(np.abs(H.indices - np.repeat(np.arange(H.shape[0]), lens))), 1))
    c_lo = np.maximum(rows[:-1] - hmax, 0)
    col16 = (H.indices - np.repeat(c_lo, np.diff(bounds))).astype(np.uint16)
    rowlen = np.array([lens[a] if len(set(lens[a:b])) == 1 else -1
                       for a, b in zip(rows[:-1], rows[1:])])
    return col16, rowlen, bounds, rows


def tridiagonal(n):
    return sps.diags([np.ones(n - 1), 2.0 * np.ones(n), np.ones(n - 1)], [-1, 0, 1], format="csr")


def pentadiagonal(n):
    return sps.diags([np.ones(n - 2), np.ones(n - 1), 4.0 * np.ones(n), np.ones(n - 1),
                      np.ones(n - 2)], [-2, -1, 0, 1, 2], format="csr")


def blocks(n, b):
    return sps.block_diag([np.ones((b, b))] * (n // b), format="csr")


def longer_row_between(n):
    i = n // 2
    return (tridiagonal(n) + sps.csr_matrix(([0.5, 0.5], ([i, i + 2], [i + 2, i])),
                                            shape=(n, n))).tocsr()


def flags(H):
    col16, rowlen, bounds, _ = tables(H)
    return cg_fused.shifted_tiles_np(col16, rowlen, bounds), rowlen


@pytest.mark.parametrize("n", [2100, 2733])
def test_tridiagonal_interior_tiles_are_flagged_the_edge_tiles_are_not(n):
    shifted, rowlen = flags(tridiagonal(n))
    assert len(rowlen) >= 3 and rowlen[0] == -1 and rowlen[-1] == -1
    assert set(rowlen[1:-1]) == {3}
    assert not shifted[0] and not shifted[-1] and shifted[1:-1].all()


def test_diagonal_is_flagged_everywhere():
    shifted, rowlen = flags(sps.identity(4000, format="csr"))
    assert set(rowlen) == {1} and shifted.all()


@pytest.mark.parametrize("b", [2, 4])
def test_diagonal_blocks_are_uniform_but_not_shifted(b):
    shifted, rowlen = flags(blocks(4000, b))
    assert set(rowlen) == {b} and not shifted.any()


def test_pentadiagonal_forms_its_columns_and_keeps_its_value_order():
    H = pentadiagonal(2000)
    col16, rowlen, bounds, _ = tables(H)
    shifted = cg_fused.shifted_tiles_np(col16, rowlen, bounds)
    assert 5 in set(rowlen) and np.array_equal(shifted, rowlen == 5)
    gmap = cg_fused.rowmajor_tiles_map_np(rowlen, shifted, bounds)
    assert np.array_equal(gmap, np.arange(H.nnz))


def test_two_longer_rows_switch_off_their_tile_alone():
    H = longer_row_between(4000)
    col16, rowlen, bounds, rows = tables(H)
    shifted = cg_fused.shifted_tiles_np(col16, rowlen, bounds)
    mid = int(np.searchsorted(rows, 2000, side="right")) - 1
    assert 0 < mid < len(rowlen) - 1 and rowlen[mid] == -1
    want = np.ones(len(rowlen), dtype=bool)
    want[[0, mid, len(rowlen) - 1]] = False
    assert np.array_equal(shifted, want)


def test_a_uniform_tile_with_one_entry_out_of_place_is_not_flagged():
    col16, rowlen, bounds, _ = tables(tridiagonal(2733))
    assert cg_fused.shifted_tiles_np(col16, rowlen, bounds)[1]
    for j in (bounds[1] + 1, bounds[2] - 1):
        moved = col16.copy()
        moved[j] += 1
        got = cg_fused.shifted_tiles_np(moved, rowlen, bounds)
        assert not got[1] and got[2:-1].all()


def test_empty_tiles_and_empty_patterns_are_not_flagged():
    assert not cg_fused.shifted_tiles_np(np.zeros(0, np.uint16), [0, -1], [0, 0, 0]).any()
    # (an empty tile between two flagged ones)
    got = cg_fused.shifted_tiles_np(np.array([5, 6, 7, 8], np.uint16), [1, 0, 1], [0, 2, 2, 4])
    assert got.tolist() == [True, False, True]


@pytest.mark.parametrize("make,n", [(tridiagonal, 2100), (tridiagonal, 2733),
                                    (longer_row_between, 4000), (lambda n: blocks(n, 4), 4000),
                                    (lambda n: sps.identity(n, format="csr"), 4000)],
                         ids=["tridiagonal-2100", "tridiagonal-2733", "longer-row-between",
                              "blocks-of-4", "diagonal"])
def test_gather_map(make, n):
    H = make(n)
    col16, rowlen, bounds, _ = tables(H)
    shifted = cg_fused.shifted_tiles_np(col16, rowlen, bounds)
    gmap = cg_fused.rowmajor_tiles_map_np(rowlen, shifted, bounds)
    nnz = H.nnz
    assert np.array_equal(np.sort(gmap), np.arange(nnz))           # a permutation
    valT = np.arange(nnz)[gmap]
    for t, (s, e) in enumerate(zip(bounds[:-1], bounds[1:])):
        if not shifted[t]:
            assert np.array_equal(valT[s:e], np.arange(s, e)), t    # the identity
            continue
        rl = rowlen[t]
        assert 1 <= rl <= cg_fused.ROWT_MAX_RL
        nrows = (e - s) // rl
        for k in range(rl):
            # valT[s + k nrows + i] = val[s + i rl + k]
            assert np.array_equal(valT[s + k * nrows:s + (k + 1) * nrows],
                                  s + np.arange(nrows) * rl + k), (t, k)
