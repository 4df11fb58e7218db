"""The two kernels of the two-launch projected-CG iteration at the edges of their addressing:
k_step1_solve_tail (csrc/banded.hip) takes every global access from a base advanced to the
workgroup's window, span or own variables plus a clamped 32-bit lane offset; k_cg_step2_hp
(csrc/cg.hip) sums the rows of a tile whose rows all have one length without row pointers and
forms its products without a test per entry.

Each kernel is compared BIT FOR BIT with the twin the project already holds to its bits, whose
kernels share no text with it:

* k_step1_solve_tail: the three-launch form, k_cg_step1_ar + k_solve_pcr with its tail
  (``_Loop(..., fused_projection=False)``), as tests/test_gpu_cg_fused_projection.py does it;
* k_cg_step2_hp: the vector step2 (k_cg_step2) followed by the CSR SpMV (k_csr_spmv) -- a loop
  object built with ``fuse_halo`` answering 0, so that only this half of the iteration differs.

x, p, r (which holds g between iterations), Hp, v, the partial arrays and the state block after
1, 2 and 5 iterations from the same primed state.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sps
import torch

from banded_setup import BandedInstance
import test_gpu_cg_fused_projection as fp

pytestmark = pytest.mark.gpu
ITERATIONS = (1, 2, 5)
WAVE, LANES = 64, 512                   # k_step1_solve_tail: one window row per lane of 512


# --------------------------------------------------------------------------------- the problems
def chain(m, bw, shift, share, seed):
    """Row i of A: ``bw`` entries +-1 from column i shift on; bw - shift = 1 column is shared
    with the next row, where both entries are +-``share``: A A' is tridiagonal with the constant
    diagonal bw - 2 + 2 share^2 and couplings c0 = share^2 / diagonal of it.  A level of the
    cyclic reduction takes the coupling c to c^2 / (1 - 2 c^2), and the factorization stops at
    the first level that leaves less than 2^-56: c0 decides the level, and with it the window
    R = rows + 2 x 2^level."""
    assert bw - shift == 1
    rng = np.random.default_rng(seed)
    n = (m - 1) * shift + bw
    assert n % 2 == 0                      # (the pair tail's loads)
    cols = (np.arange(m)[:, None] * shift + np.arange(bw)[None, :]).ravel()
    val = rng.choice([-1.0, 1.0], m * bw).reshape(m, bw)
    val[:, 0] *= share
    val[:, -1] *= share
    A = sps.csr_matrix((val.ravel(), (np.repeat(np.arange(m), bw), cols)), shape=(m, n))
    A.sort_indices()
    off = rng.uniform(-0.4, 0.4, n - 1)
    H = sps.diags([off, rng.uniform(1.5, 2.5, n), off], [-1, 0, 1], format="csr")
    return A, H, rng.standard_normal(n)


# name -> (constructor of (A, H, c), whole waves of the 8 without a window row or None); 260
# rows per workgroup in all of them (the factorization offers no other count at these sizes),
# so the window is R = 260 + 2 x 2^level rows and a multiple of 64 does not occur:
# R = 388 = 6 x 64 + 4 (level 6) and R = 324 = 5 x 64 + 4 (level 5) are the nearest -- the last
# wave with rows holds four.  No geometry leaves 0 waves idle either (that needs level 7,
# R = 516 > 512 lanes, which the kernel's launcher refuses): level 6, one idle wave, is the
# fullest.
WINDOWS = {
    # m smaller than one window: one workgroup, its window cut at both edges of the matrix
    "one-window": (lambda: banded(2000, 200), None),
    # the last window reaches past row m: a third workgroup that owns one row
    "past-m": (lambda: banded(5210, 521), None),
    "level-6": (lambda: chain(701, 4, 3, 2.0 ** 0.5, 10), 1),   # c0 = 1 / 3: R = 388
    # tests/pcr_family_cases.py: strided_rows(1301, 4, 6), c0 about 1 / 4: R = 324
    "level-5": (lambda: family_rows(), 2),
    "level-4": (lambda: chain(701, 8, 7, 0.5, 12), 3),          # c0 = 1 / 26: R = 292
}


def banded(n, m):
    inst = BandedInstance(n, m)
    return inst.A.tocsr(), inst.H.tocsr(), inst.c


def family_rows():
    import pcr_family_cases as cases
    bw, stride2, m = cases.TAIL_WIDTHS[2]
    return cases.strided_rows(m, bw, stride2)


@functools.lru_cache(maxsize=None)
def window_problem(name):
    A, H, c = WINDOWS[name][0]()
    return fp.Problem(A.tocsr(), H.tocsr(), c)


def tridiagonal(n, seed):
    rng = np.random.default_rng(seed)
    off = rng.uniform(-0.4, 0.4, n - 1)
    return sps.diags([off, rng.uniform(1.5, 2.5, n), off], [-1, 0, 1], format="csr")


def pentadiagonal(n):
    rng = np.random.default_rng(5)
    o1, o2 = rng.uniform(-0.4, 0.4, n - 1), rng.uniform(-0.3, 0.3, n - 2)
    return sps.diags([o2, o1, rng.uniform(2.5, 3.5, n), o1, o2], [-2, -1, 0, 1, 2], format="csr")


def one_longer_row(n):
    """Tridiagonal, and rows n / 2 and n / 2 + 2 (in a middle tile) hold a fourth entry."""
    i = n // 2
    H = tridiagonal(n, 6) + sps.csr_matrix(([0.2, 0.2], ([i, i + 2], [i + 2, i])), shape=(n, n))
    H = H.tocsr()
    H.sort_indices()
    return H


def pairs(n):
    """2 x 2 diagonal blocks: two entries in EVERY row (no short first or last row), 1024 rows per
    tile of 2048 entries -- the (Q, QS) = (4, 5) instantiations."""
    rng = np.random.default_rng(8)
    off = np.zeros(n - 1)
    off[0::2] = rng.uniform(-0.4, 0.4, n // 2)
    H = sps.diags([off, rng.uniform(1.5, 2.5, n), off], [-1, 0, 1], format="csr")
    H.eliminate_zeros()
    H.sort_indices()
    return H


# name -> (n, Hessian or None for the instance's own, (Q, QS) of the launch)
HESSIANS = {
    # 3 row tiles; the first and the last hold a short row (irregular), the middle one is uniform
    "tridiagonal-2000": (2000, None, (3, 3)),
    "pentadiagonal": (2000, pentadiagonal, (3, 3)),
    "one-longer-row": (4000, one_longer_row, (3, 3)),
    "short-last-tile": (None, None, (3, 3)),                  # n: see short_last_tile_n
    "pairs": (4000, pairs, (4, 5)),
}


def tile_rows(H):
    import ipsolver.device as dv
    pat = dv.DeviceCSR.from_scipy(H).pattern
    return np.diff(pat.tiles_h[:pat.ntiles + 1])


@functools.lru_cache(maxsize=None)
def short_last_tile_n():
    """The smallest even n >= 1400 whose tridiagonal Hessian ends in a tile of fewer than 64
    rows (the tiles are cut by entries: about 682 rows each)."""
    for n in range(1400, 2200, 2):
        if tile_rows(tridiagonal(n, 7))[-1] < WAVE:
            return n
    raise AssertionError("no n with a last tile of fewer than 64 rows")


@functools.lru_cache(maxsize=None)
def hessian_problem(name):
    n, make, _ = HESSIANS[name]
    if name == "short-last-tile":
        n, make = short_last_tile_n(), lambda k: tridiagonal(k, 7)
    inst = BandedInstance(n, n // 10)
    H = inst.H.tocsr() if make is None else make(n)
    return fp.Problem(inst.A.tocsr(), H.tocsr(), inst.c)


# ------------------------------------------------------------------------------------ the runs
def arm_guard(L, q):
    """The radius guard as ipsolver.cg_fused.projected_cg arms it for x0 = 0: X0 = 0, Q0 >= ||g0||."""
    from ipsolver import _hip
    lib = _hip.load()
    L.rguard.copy_(torch.tensor([0.0, lib.ipx_rguard_start(q.rt_g), 0.0], dtype=torch.float64))
    L.args.radius_guard = 1


def snapshots(L, q, radius, guard=False):
    """{iterations: {field: tensor}} at ITERATIONS, one batch after the other."""
    fp.prime(L, q, radius)
    if guard:
        arm_guard(L, q)
    import ipsolver.device as dv
    from ipsolver import _hip
    lib, st = _hip.load(), dv.stream_ptr()
    out, it = {}, 0
    nH = int(L.args.H_ntiles)
    for k in ITERATIONS:
        _hip.check(lib.ipx_cg_iterate(L.ref(), it, k, st), "ipx_cg_iterate")
        it = k
        torch.cuda.synchronize()
        snap = {name: getattr(L, name).clone() for name in ("x", "p", "r", "Hp", "v", "state")}
        nwin = L.geometry[2]
        snap["part1"] = L.part1[:2 * nH].clone()             # y'y, p'y per row tile of H
        snap["part3"] = L.part3[:2 * nwin].clone()
        snap["part4"] = L.part4[:nwin].clone()
        out[k] = snap
    import ipsolver.cg_fused as cg_fused
    s = L.state.tolist()
    assert int(s[cg_fused.ST_STOP]) == 0 and int(s[cg_fused.ST_IT_DONE]) == ITERATIONS[-1]
    return out


def assert_same_bits(got, want):
    for k in ITERATIONS:
        for name in want[k]:
            a, b = got[k][name], want[k][name]
            # (bits, not values: a NaN or a signed zero must be the twin's too)
            assert torch.equal(a.view(torch.int64), b.view(torch.int64)), (k, name)


# ---------------------------------------------------------------------------- k_step1_solve_tail
def idle_waves(L):
    R = L.geometry[1] + 2 * (1 << L.pcr_L)
    assert L.geometry[1] == 260 and R <= LANES
    return LANES // WAVE - -(-R // WAVE)


def test_windows_leave_one_two_and_three_waves_without_rows(monkeypatch):
    """The geometries the cases below stand for: what WINDOWS says of each."""
    for name, (_, idle) in sorted(WINDOWS.items()):
        if idle is not None:
            assert idle_waves(fp.loop(monkeypatch, window_problem(name), True)) == idle, name


@pytest.mark.parametrize("mode", ["guard", "inf", "carried", "read-xn2"])
@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_solve_tail_against_three_launches(monkeypatch, name, mode):
    """XN = 3 (the benchmark's), 1, 2 and 0 of the one-launch projection against k_cg_step1_ar +
    k_solve_pcr, on windows cut at the matrix edges and with 1, 2 and 3 waves beyond the window."""
    q = window_problem(name)
    radius = np.inf if mode == "inf" else 1e300
    runs = []
    for fused in (True, False):
        L = fp.loop(monkeypatch, q, fused, read_xn2=mode == "read-xn2")
        assert fp.bound(L) == fused
        runs.append(snapshots(L, q, radius, guard=mode == "guard"))
        if fused:
            if name == "one-window":
                assert q.m < L.geometry[1] and L.geometry[2] == 1
            if name == "past-m":
                assert L.geometry[2] * L.geometry[1] > q.m > (L.geometry[2] - 1) * L.geometry[1]
    assert_same_bits(*runs)


# --------------------------------------------------------------------------------- k_cg_step2_hp
def hp_loop(monkeypatch, q, fused_hp):
    """The two-launch loop, or its twin whose second half is k_cg_step2 + k_csr_spmv."""
    import ipsolver.cg_fused as cg_fused
    if not fused_hp:
        monkeypatch.setattr(cg_fused, "fuse_halo", lambda pattern: 0)
    monkeypatch.setenv("IPX_DEBUG_FORMS", "no-resident")
    L = cg_fused._Loop(q.H, q.P, None, None, resident=False, fused_projection=True)
    assert not L.args.resident and fp.bound(L)
    assert (L.args.H_hmax > 0) == fused_hp and bool(L.args.xsums) == fused_hp
    return L


@pytest.mark.parametrize("mode", ["guard", "inf", "carried"])
@pytest.mark.parametrize("name", sorted(HESSIANS))
def test_step2_hp_against_step2_and_spmv(monkeypatch, name, mode):
    """GUARD (the benchmark's), the plain and the XSUM instantiation against the vector step2
    followed by the CSR SpMV: tiles with and without one row length in one launch, a longer row
    in a middle tile, a last tile of fewer than 64 rows, and the wider (Q, QS) pair."""
    q = hessian_problem(name)
    pat = q.H.pattern
    rows = np.diff(pat.tiles_h[:pat.ntiles + 1])
    lens = np.diff(pat.indptr_h)
    uniform = [len(set(lens[a:b])) == 1 for a, b in zip(np.cumsum(rows) - rows, np.cumsum(rows))]
    if name == "tridiagonal-2000":
        assert uniform == [False, True, False]
    if name == "pentadiagonal":
        assert sorted(set(lens)) == [3, 4, 5] and any(uniform)
    if name == "one-longer-row":
        mid = int(np.searchsorted(np.cumsum(rows), q.n // 2, side="right"))
        assert 0 < mid < len(rows) - 1 and not uniform[mid] and any(uniform)
        assert sorted(set(lens[1:-1])) == [3, 4]
    if name == "short-last-tile":
        assert rows[-1] < WAVE
    if name == "pairs":
        assert all(uniform) and set(lens) == {2}
    Q = -(-int(rows.max()) // 256)
    assert (3 if Q <= 3 else 4) == HESSIANS[name][2][0], rows
    radius = np.inf if mode == "inf" else 1e300
    runs = []
    for fused_hp in (True, False):
        L = hp_loop(monkeypatch, q, fused_hp)
        # (the twin has no carried sums and no guard: it reads x and p for the radius test)
        runs.append(snapshots(L, q, radius, guard=mode == "guard" and fused_hp))
    assert_same_bits(*runs)
