"""k_cg_step2_hp (csrc/cg.hip) on row tiles whose rows all have one short length -- the tiles a
banded Hessian is made of -- beside the irregular tiles at its edges, in every form the loop can
take: plain (trust_radius = inf), GUARD (a finite radius under the radius guard), XSUM (a finite
radius with the carried sums, debug form ``no-radius-guard``) and BOX.

Each run is compared BIT FOR BIT with the twin tests/test_gpu_loop_kernel_edges.py uses: the
vector k_cg_step2 followed by k_csr_spmv, on a loop object whose ``fuse_halo`` answers 0, so that
only this half of the iteration differs.  x, p, r (which holds g between iterations), Hp, v, the
partial arrays and the state block after 1, 2 and 5 iterations from one primed state.

The Hessians (n between 2 000 and 6 000; the tiles are cut by entries, 2 048 to a tile, and by
rows, 1 024 to a tile; ``rowlen`` is what ipsolver.cg_fused.compact_columns hands the kernel,
the tile's common row length or -1):

* tridiagonal at n = 2 100, 2 732 and 2 733: an irregular first and last tile (their edge rows
  hold two entries) beside uniform interior ones of 682 or 683 rows, fewer than the 768 lanes'
  rows; an odd n keeps the projection on its three launches;
* 2 x 2 and 4 x 4 symmetric blocks on the diagonal, and the diagonal alone: two, four and one
  entry in EVERY row, so that tile 0 and the last tile are uniform too and their spans end at
  column 0 and column n; the diagonal and the pairs run the (Q, QS) = (4, 5) instantiations;
* pentadiagonal: five entries per interior row;
* tridiagonal with two rows of four entries in a middle tile: an irregular tile between two
  uniform ones;
* tridiagonal with a further diagonal passed as a vector of its own (HAS_DIAG);
* tridiagonal over a Jacobian that leaves 64 columns untouched, with c zero there: x, r and p
  stay exact zeros deep inside that range for five iterations, and two blocks of rows there hold
  only negative and only positive entries -- whatever the sign of the zeros of p, in one of the
  blocks every product of a row is -0.0, and the row sum has to be the twin's +0.0 (a sum that
  starts from 0.0: 0.0 + -0.0 = +0.0).
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sps

from banded_setup import BandedInstance
import test_gpu_cg_fused_projection as fp
import test_gpu_loop_kernel_edges as edges

pytestmark = pytest.mark.gpu
GAP = 64                               # columns the Jacobian of "signed-zeros" leaves untouched


# ------------------------------------------------------------------------------- the Hessians
def blocks(n, b, seed):
    """Symmetric b x b blocks on the diagonal, every entry of a block stored: b per row."""
    assert n % b == 0
    rng = np.random.default_rng(seed)
    B = rng.uniform(-0.3, 0.3, (n // b, b, b))
    B = B + B.transpose(0, 2, 1)
    B[:, np.arange(b), np.arange(b)] = rng.uniform(2.5, 3.5, (n // b, b))
    H = sps.block_diag(list(B), format="csr")
    H.sort_indices()
    assert H.nnz == n * b
    return H


def diagonal(n):
    return sps.diags([np.random.default_rng(9).uniform(1.5, 2.5, n)], [0], format="csr")


def longer_row_between(n):
    """Tridiagonal, and rows n / 2 and n / 2 + 2 hold a fourth entry (symmetric)."""
    i = n // 2
    H = edges.tridiagonal(n, 16) + sps.csr_matrix(([0.15, 0.15], ([i, i + 2], [i + 2, i])),
                                                  shape=(n, n))
    H = H.tocsr()
    H.sort_indices()
    return H


def gap_start(m):
    return (m // 2 - 1) * 3 + 4


def signed_zeros(m):
    """(A, H, c): edges.chain's Jacobian with the columns of its rows from m / 2 on moved GAP
    columns to the right (A A' stays tridiagonal, one coupling is zero), a tridiagonal H whose
    rows g + 12 .. g + 28 hold only negative and rows g + 34 .. g + 50 only positive entries
    (g: first untouched column), c zero on the untouched columns."""
    A, _, c0 = edges.chain(m, 4, 3, 2.0 ** 0.5, 21)
    A = A.tocsr()
    g = gap_start(m)
    cols = A.indices.copy().reshape(m, 4)
    assert cols[m // 2 - 1].max() == g - 1 and cols[m // 2].min() == g - 1
    # (the rows share a column with their neighbour; the shift undoes that at the gap)
    cols[m // 2:] += GAP + 1
    n = int(cols.max()) + 2
    assert n % 2 == 0
    A = sps.csr_matrix((A.data, cols.ravel(), A.indptr), shape=(m, n))
    rng = np.random.default_rng(22)
    off = rng.uniform(-0.4, 0.4, n - 1)
    d = rng.uniform(1.5, 2.5, n)
    off[g + 11:g + 29] = -np.abs(off[g + 11:g + 29]) - 0.05
    d[g + 12:g + 29] *= -1.0
    off[g + 33:g + 51] = np.abs(off[g + 33:g + 51]) + 0.05
    H = sps.diags([off, d, off], [-1, 0, 1], format="csr")
    c = rng.standard_normal(n)
    c[g:g + GAP] = 0.0
    return A, H, c


# name -> (n, Hessian(n) or None for the tridiagonal of that seed, Q of the launch,
#          what rowlen must look like)
def _interior(rl):
    return lambda r: r[0] == -1 and r[-1] == -1 and len(r) >= 3 and set(r[1:-1]) == {rl}


CASES = {
    "tridiagonal-2100": (2100, None, 3, _interior(3)),
    "tridiagonal-2732": (2732, None, 3, _interior(3)),
    "tridiagonal-2733": (2733, None, 3, _interior(3)),
    "pairs": (4000, edges.pairs, 4, lambda r: set(r) == {2}),
    "diagonal": (4000, diagonal, 4, lambda r: set(r) == {1}),
    "blocks-of-4": (4000, lambda n: blocks(n, 4, 13), 3, lambda r: set(r) == {4}),
    "pentadiagonal": (2000, edges.pentadiagonal, 3, lambda r: 5 in set(r)),
    "longer-row-between": (4000, longer_row_between, 3,
                           lambda r: any(a == 3 and b == -1 and c == 3
                                         for a, b, c in zip(r[:-2], r[1:-1], r[2:]))),
    "separate-diagonal": (2732, None, 3, _interior(3)),
    "signed-zeros": (None, None, 3, _interior(3)),
}
M_ZEROS = 701


@functools.lru_cache(maxsize=None)
def problem(name):
    n, make, _, _ = CASES[name]
    if name == "signed-zeros":
        A, H, c = signed_zeros(M_ZEROS)
        return fp.Problem(A.tocsr(), H.tocsr(), c)
    inst = BandedInstance(n, n // 10)
    H = edges.tridiagonal(n, 17) if make is None else make(n)
    q = fp.Problem(inst.A.tocsr(), H.tocsr(), inst.c)
    if name == "separate-diagonal":
        import ipsolver.device as dv
        from ipsolver.operators import DeviceHessian
        extra = np.random.default_rng(18).uniform(0.1, 0.9, n)
        # (merge=False: the diagonal stays a vector of its own, as in an SQP's outer iterations)
        q.H = DeviceHessian(n, csr=q.H, diag=dv.DVec.from_host(extra), merge=False)
    return q


def csr_of(q):
    return getattr(q.H, "csr", q.H)


def rowlen_of(q):
    import ipsolver.cg_fused as cg_fused
    pat = csr_of(q).pattern
    hmax = cg_fused.fuse_halo(pat)
    assert hmax > 0
    return [int(t) for t in cg_fused.compact_columns(pat, hmax)[1].cpu().tolist()]


# ------------------------------------------------------------------------------------ the runs
FORMS = {"inf": "no-resident", "guard": "no-resident", "xsum": "no-resident,no-radius-guard",
         "box": "no-resident"}


def hp_loop(monkeypatch, q, fused_hp, form):
    """The separate-launch loop, or its twin whose second half is k_cg_step2 + k_csr_spmv."""
    import ipsolver.cg_fused as cg_fused
    import ipsolver.device as dv
    if not fused_hp:
        monkeypatch.setattr(cg_fused, "fuse_halo", lambda pattern: 0)
    monkeypatch.setenv("IPX_DEBUG_FORMS", FORMS[form])
    lb = ub = None
    if form == "box":
        lb, ub = dv.DVec.full(q.n, -1e3), dv.DVec.full(q.n, 1e3)
    L = cg_fused._Loop(q.H, q.P, lb, ub, resident=False, fused_projection=q.n % 2 == 0)
    a = L.args
    assert not a.resident and (a.H_hmax > 0) == fused_hp and bool(a.lb) == (form == "box")
    if form != "box":
        assert bool(a.xsums) == fused_hp and bool(a.A_span)
    if fused_hp:
        assert bool(a.H_col16) and bool(a.H_rowlen) and bool(a.H_diag) == hasattr(q.H, "csr")
    return L


def run_pair(monkeypatch, q, form):
    radius = np.inf if form == "inf" else 1e300
    runs = []
    for fused_hp in (True, False):
        L = hp_loop(monkeypatch, q, fused_hp, form)
        # (the twin has no carried sums and no guard: it reads x and p for the radius test)
        runs.append(edges.snapshots(L, q, radius, guard=form == "guard" and fused_hp))
    edges.assert_same_bits(*runs)
    return runs[0]


@pytest.mark.parametrize("form", ["inf", "guard", "xsum"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_uniform_short_rows_against_step2_and_spmv(monkeypatch, name, form):
    q = problem(name)
    pat = csr_of(q).pattern
    rows = np.diff(pat.tiles_h[:pat.ntiles + 1])
    rl = rowlen_of(q)
    assert CASES[name][3](rl), rl
    assert (3 if -(-int(rows.max()) // 256) <= 3 else 4) == CASES[name][2], rows
    if name.startswith("tridiagonal"):
        # lanes beyond the rows of a uniform tile; 3 or more tiles
        assert all(r < 3 * 256 and r % 64 for r, k in zip(rows, rl) if k == 3)
    got = run_pair(monkeypatch, q, form)
    if name == "signed-zeros":
        assert_minus_zero_products(q, got, rows, rl)


def assert_minus_zero_products(q, got, rows, rl):
    """The case is what its name says: after every batch, a uniform tile holds rows whose
    products with p are all -0.0, and Hp is +0.0 there."""
    H = csr_of(q)
    pat = H.pattern
    indptr, indices = pat.indptr_h.astype(np.int64), pat.indices_h.astype(np.int64)
    val = H.val.cpu().numpy()
    g = gap_start(M_ZEROS)
    first = np.cumsum(rows) - rows
    tile = int(np.searchsorted(first, g + 12, side="right")) - 1
    assert rl[tile] == 3 and first[tile] + rows[tile] > g + 51
    for k in edges.ITERATIONS:
        p, Hp = got[k]["p"].cpu().numpy(), got[k]["Hp"].cpu().numpy()
        found = 0
        for i in list(range(g + 12, g + 29)) + list(range(g + 34, g + 51)):
            prods = val[indptr[i]:indptr[i + 1]] * p[indices[indptr[i]:indptr[i + 1]]]
            assert np.all(prods == 0.0) and Hp[i] == 0.0 and not np.signbit(Hp[i]), (k, i)
            found += bool(np.all(np.signbit(prods)))
        assert found >= 17, (k, found)


@pytest.mark.parametrize("name", ["tridiagonal-2732", "pairs"])
def test_uniform_short_rows_in_a_box(monkeypatch, name):
    """BOX: bounds far from the iterates (no violation is counted), vector step1."""
    run_pair(monkeypatch, problem(name), "box")
