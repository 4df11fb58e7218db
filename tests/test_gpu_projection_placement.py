"""Where the windows of the cyclic-reduction solve run, and rows of A without column offsets.

The kernels of csrc/banded.hip that work on the solve's windows (k_solve_pcr, k_step1_solve_tail)
take their window from ``ipx_xcd_item(blockIdx.x, nwin)`` on a grid padded to a multiple of 8, so
that neighbouring windows -- whose halo rows are each other's own rows -- run on one XCD.  Which
window computes what, where its partials land and the order of every sum are unchanged, so every
form must agree BIT FOR BIT with every other; the padding workgroups must store nothing, and the
partial count handed back must be the window count, not the grid.

Window counts (260 rows per window): 7 (fewer windows than XCDs), 8, 9 (grid 16: seven padding
workgroups), 18 (the last window owns one row), 25.

Contiguous rows (ipx_cg_args.A_contig): where entry k of every row of A sits at the row's first
column + k, k_step1_solve_tail takes the offset as a constant and does not read the 16-bit table;
debug form ``table-columns`` keeps the table.  A pattern with one gap per row clears the flag.
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sps
import torch

from banded_setup import BandedInstance

pytestmark = pytest.mark.gpu
ROWS_WG = 260
SIZES = [1820, 2080, 2340, 4421, 6500]          # m; n = 10 m
WINDOWS = {1820: 7, 2080: 8, 2340: 9, 4421: 18, 6500: 25}
BATCHES = (1, 16, 7)
FIELDS = ("x", "r", "p", "Hp", "v", "state")
SENTINEL = -7.25


class Problem:
    """Device operators, projections and the host-primed start (x0 = 0, r0 = Z c, g0 = Z r0) of
    one instance: computed once and shared, never written to."""

    def __init__(self, A, H, c):
        import ipsolver.device as dv
        import ipsolver.projector as proj
        self.n, self.m = A.shape[1], A.shape[0]
        self.A_host = A
        self.A = dv.DeviceCSR.from_scipy(A)
        self.H = dv.DeviceCSR.from_scipy(H)
        self.Z, _, self.Y = proj.projections(self.A)
        self.P = self.Z.projector
        self.c = dv.DVec.from_host(c)
        self.r0 = self.Z.dot(self.c)
        self.g0 = self.Z.dot(self.r0)
        self.rt_g = self.g0.sumsq_amax()[0]
        torch.cuda.synchronize()


def problem(m, variant="plain"):
    return _problem(m, variant)


@functools.lru_cache(maxsize=None)
def _problem(m, variant):
    n = 10 * m
    inst = BandedInstance(n, m)
    A, H = inst.A.tocsr(), inst.H.tocsr()
    A.sort_indices()
    if variant == "gap":
        # 15 entries per row, the last one a column further on.  Not in the last row of a
        # window (nor of the matrix, which has no column there): the column it leaves would be
        # owned by the next window and the one it takes by this one, and the tail of the solve
        # wants the owners non-decreasing along the variables (cg_fused.fuse_vown) -- such a
        # pattern runs the separate launches in every form.
        assert set(np.diff(A.indptr)) == {15}
        cols = A.indices.reshape(m, 15).copy()
        assert np.array_equal(cols - cols[:, :1], np.broadcast_to(np.arange(15), cols.shape))
        move = (cols[:, -1] + 1 < n) & (np.arange(m) % ROWS_WG != ROWS_WG - 1)
        assert move.sum() >= m - m // ROWS_WG - 1
        cols[move, -1] += 1
        A = sps.csr_matrix((A.data.copy(), cols.ravel(), A.indptr.copy()), shape=A.shape)
        A.sort_indices()
    return Problem(A, H, inst.c)


def loop(monkeypatch, q, fused, forms="no-resident"):
    import ipsolver.cg_fused as cg_fused
    monkeypatch.setenv("IPX_DEBUG_FORMS", forms)
    L = cg_fused._Loop(q.H, q.P, None, None, resident=False, fused_projection=fused)
    assert not L.args.resident and L.args.A_span > 0 and L.args.H_hmax > 0 and L.args.At_qv > 0
    assert L.args.fused_proj == (1 if fused else 0)
    return L


def prime(L, q, radius=1e300, tol=0.0):
    import ipsolver.cg_fused as cg_fused
    import ipsolver.device as dv
    from ipsolver import _hip
    st = dv.stream_ptr()
    L.args.no_radius = 1 if np.isinf(radius) else 0
    L.x.zero_()
    L.r.copy_(q.r0.t)
    _hip.call("ipx_axpby", q.n, -1.0, dv._p(q.g0.t), 0.0, None, dv._p(L.p), st)
    init = np.zeros(L.state.numel())
    init[cg_fused.ST_RTG0] = q.rt_g
    init[cg_fused.ST_TOL] = tol
    init[cg_fused.ST_RADIUS] = radius
    init[cg_fused.ST_ORTH_RHS] = q.P.orth_tol * q.P.norm_A
    L.state.copy_(torch.from_numpy(init))
    _hip.check(_hip.load().ipx_cg_hp(L.ref(), st), "ipx_cg_hp")


def run(monkeypatch, q, fused, forms="no-resident"):
    """The loop's vectors, state block and partials after batches of 1, 16 and 7 iterations.
    part3 / part4 beyond what the window count accounts for are filled with a sentinel first:
    a padding workgroup that stored anything would overwrite it."""
    import ipsolver.cg_fused as cg_fused
    import ipsolver.device as dv
    from ipsolver import _hip
    L = loop(monkeypatch, q, fused, forms)
    nwin = L.geometry[2]
    prime(L, q)
    L.part3[2 * nwin:].fill_(SENTINEL)
    L.part4[nwin:].fill_(SENTINEL)
    lib, st = _hip.load(), dv.stream_ptr()
    snaps, it = [], 0
    for k in BATCHES:
        _hip.check(lib.ipx_cg_iterate(L.ref(), it, it + k, st), "ipx_cg_iterate")
        it += k
        torch.cuda.synchronize()
        s = {name: getattr(L, name).clone() for name in FIELDS}
        s["part3"], s["part4"] = L.part3[:nwin].clone(), L.part4[:nwin].clone()
        s["beyond3"], s["beyond4"] = L.part3[2 * nwin:].clone(), L.part4[nwin:].clone()
        snaps.append(s)
    assert int(L.state[cg_fused.ST_STOP].item()) == 0
    assert int(L.state[cg_fused.ST_IT_DONE].item()) == sum(BATCHES)
    return L, snaps


_RUNS = {}


def cached_run(monkeypatch, m, fused, forms="no-resident", variant="plain"):
    key = (m, fused, forms, variant)
    if key not in _RUNS:
        L, snaps = run(monkeypatch, problem(m, variant), fused, forms)
        _RUNS[key] = (dict(geometry=L.geometry, contig=int(L.args.A_contig),
                           off16=bool(L.args.A_ell_off16)), snaps)
    return _RUNS[key]


def assert_same(sa, sb, what):
    for k, (a, b) in enumerate(zip(sa, sb)):
        for name in FIELDS + ("part3", "part4"):
            assert torch.equal(a[name], b[name]), (what, "batch %d" % k, name)


@pytest.mark.parametrize("m", SIZES)
def test_fused_launch_against_three_launches(monkeypatch, m):
    """k_step1_solve_tail against k_cg_step1_ar + k_solve_pcr with its tail, both on the XCD
    map: the same bits after 1, 17 and 24 iterations; nothing stored beyond the window count."""
    info_f, fused = cached_run(monkeypatch, m, True)
    info_3, three = cached_run(monkeypatch, m, False)
    assert info_f["geometry"] == (True, ROWS_WG, WINDOWS[m]) == info_3["geometry"]
    assert info_f["contig"] == 1 and info_f["off16"]
    assert_same(fused, three, "fused against three launches")
    for snaps in (fused, three):
        for s in snaps:
            assert bool((s["beyond3"] == SENTINEL).all()) and bool((s["beyond4"] == SENTINEL).all())


@pytest.mark.parametrize("m", SIZES)
def test_contiguous_rows_against_the_table(monkeypatch, m):
    """On these instances the flag is set; the launch that takes the offsets as constants and
    the one that reads the table (``table-columns``) leave the same bits."""
    import ipsolver.cg_fused as cg_fused
    q = problem(m)
    info_c, contig = cached_run(monkeypatch, m, True)
    info_t, table = cached_run(monkeypatch, m, True, "no-resident,table-columns")
    assert cg_fused.ell_contiguous(q.P.A, 15)
    assert info_c["contig"] == 1 and info_t["contig"] == 0 and info_t["off16"]
    assert_same(contig, table, "constant offsets against the table")


def test_rows_with_a_gap_keep_the_table(monkeypatch):
    """15 entries per row, the last one shifted by a column: the flag is clear, the fused launch
    reads the table and agrees with the three launches."""
    import ipsolver.cg_fused as cg_fused
    m = 2340
    q = problem(m, "gap")
    info_f, fused = cached_run(monkeypatch, m, True, variant="gap")
    info_3, three = cached_run(monkeypatch, m, False, variant="gap")
    assert not cg_fused.ell_contiguous(q.P.A, 15)
    assert info_f["contig"] == 0 and info_f["off16"]
    assert info_f["geometry"] == (True, ROWS_WG, WINDOWS[m])
    assert_same(fused, three, "rows with a gap")


@pytest.mark.parametrize("m", SIZES)
def test_partial_count_is_the_window_count(monkeypatch, m):
    """ipx_banded_solve_resid (k_solve_pcr without a tail): *npartial is the window count, the
    partials beyond it are untouched, and x solves the system.  Bound on the residual: a
    fixed-order fp64 cyclic reduction of a symmetric positive definite tridiagonal matrix is
    backward stable with a constant of a few units per level (at most 7 levels), and the
    windows drop couplings below 2^-56 of the diagonal: |w - S x| <= 1e-12 (|S| |x| + |w|)
    leaves three orders of magnitude over that, while a window computed by the wrong
    workgroup, or not at all, is wrong in the leading digit."""
    import ipsolver.device as dv
    from ipsolver import _hip
    monkeypatch.delenv("IPX_DEBUG_FORMS", raising=False)
    q = problem(m)
    nwin = WINDOWS[m]
    rng = np.random.default_rng(m)
    w = rng.standard_normal(m)
    wd = dv.DVec.from_host(w)
    x = torch.full((m,), np.nan, dtype=torch.float64, device=wd.t.device)
    part = torch.full((nwin + 24,), SENTINEL, dtype=torch.float64, device=wd.t.device)
    npart = ctypes.c_int32(0)
    _hip.call("ipx_banded_solve_resid", ctypes.c_void_p(q.P.solver.handle), dv._p(wd.t), dv._p(x),
              dv._p(part), ctypes.byref(npart), None, dv.stream_ptr())
    torch.cuda.synchronize()
    assert npart.value == nwin
    p = part.cpu().numpy()
    assert np.all(np.isfinite(p[:nwin])) and np.all(p[:nwin] >= 0.0) and np.all(p[nwin:] == SENTINEL)
    xh = x.cpu().numpy()
    assert np.all(np.isfinite(xh))
    S = (q.A_host @ q.A_host.T).tocsr()
    res = np.abs(w - S.dot(xh))
    bound = 1e-12 * (abs(S).dot(np.abs(xh)) + np.abs(w))
    print("m = %d: max |w - S x| / bound = %.3g" % (m, float(np.max(res / bound))))
    assert np.all(res <= bound)


def test_public_call_with_the_priming_projection(monkeypatch):
    """qp.projected_cg, m = 2340, 40 iterations, with and without ``no-fused-projection``: the
    same bits.  The size is below the resident kernel's limit, where the fused projection is not
    the default, so the test lowers the limit it is compared with; the second call on the same
    Jacobian object finds the ELL-transposed copy current and arms the form before the priming,
    whose two projections are then k_step1_solve_tail<.., PRIME> launches."""
    import ipsolver.cg_fused as cg_fused
    import ipsolver.qp as qp
    m = 2340
    q = problem(m)
    limits = dict(cg_fused.resident_limits(), max_wg=4)
    monkeypatch.setattr(cg_fused, "resident_limits", lambda: limits)
    armed = []
    real_arm = cg_fused._Loop.arm_fused_projection

    def recording(self, iterations=None):
        on = real_arm(self, iterations)
        armed.append(on)
        return on

    monkeypatch.setattr(cg_fused._Loop, "arm_fused_projection", recording)
    out = {}
    for forms in ("no-resident", "no-resident,no-fused-projection"):
        monkeypatch.setenv("IPX_DEBUG_FORMS", forms)
        for call in range(2):
            del armed[:]
            retries = cg_fused.STATS["prime_retries"]
            primed = cg_fused.STATS["primed_on_device"]
            x, info = qp.projected_cg(q.H, q.c, q.Z, q.Y, np.zeros(m), trust_radius=1e300, tol=0,
                                      max_iter=40)
            assert cg_fused.STATS["prime_retries"] == retries
            assert cg_fused.STATS["primed_on_device"] == primed + 1
            L = next(reversed(cg_fused._POOL.values()))
            assert L.geometry == (True, ROWS_WG, WINDOWS[m]) and not L.args.resident
            out[(forms, call)] = (x.t.clone(), info, list(armed), int(L.args.fused_proj))
    fused, three = "no-resident", "no-resident,no-fused-projection"
    assert out[(fused, 1)][2][0] is True and out[(fused, 1)][3] == 1      # armed before the priming
    assert not any(out[(three, 1)][2]) and out[(three, 1)][3] == 0
    assert out[(fused, 1)][1]["niter"] == 40
    for call in range(2):
        assert out[(fused, call)][1] == out[(three, call)][1]
        assert torch.equal(out[(fused, call)][0], out[(three, call)][0])
    assert torch.equal(out[(fused, 0)][0], out[(fused, 1)][0])


def box_schur_nine_windows():
    """tests/fuzz_box_schur.py's barrier-shaped problem at 2340 general rows (nine windows):
    (A, H, c, b, lb, keyword arguments of projected_cg)."""
    rng = np.random.default_rng(2340)
    rl, shift, m = 15, 8, 2340
    n = (m - 1) * shift + rl
    rows = np.repeat(np.arange(m), rl)
    cols = (np.arange(m)[:, None] * shift + np.arange(rl)[None, :]).ravel()
    J = sps.csr_matrix((rng.uniform(0.5, 1.5, m * rl) * rng.choice([-1.0, 1.0], m * rl),
                        (rows, cols)), shape=(m, n))
    Lo = np.arange(n)
    I = sps.eye(n, format="csr")
    s = rng.uniform(1e-6, 2.0, m + n)
    A = sps.bmat([[J, sps.diags(s[:m]), None], [-I[Lo], None, sps.diags(s[m:])]], format="csr")
    A.sort_indices()
    M, N = A.shape
    assert N <= 40000
    off = rng.uniform(-0.4, 0.4, n - 1)
    Hx = sps.diags([off, rng.uniform(1.5, 2.5, n), off], [-1, 0, 1], format="csr")
    Hz = sps.block_diag([Hx, sps.diags(rng.uniform(0.5, 2.0, N - n))], format="csr")
    c = rng.standard_normal(N)
    b = np.zeros(M)
    lb = np.concatenate((np.full(n, -np.inf), np.full(N - n, -0.995)))
    return A, Hz, c, b, lb, dict(trust_radius=np.inf, tol=1e-10, max_iter=40)


def test_box_schur_solve_on_nine_windows():
    """The Schur solve of the barrier-shaped problem (k_solve_pcr forming its own right-hand
    side, with the per-item tail) at 9 windows, through the public solver, against the host
    oracle's projected CG: tests/fuzz_box_schur.py's problem and its tolerance (the same
    iteration count and exit, x to 1e-9)."""
    import os
    import ipsolver.device as dv
    import ipsolver.projector as projector
    import ipsolver.cg_fused as cg_fused
    from ipsolver import _hip
    import oracle
    os.environ.pop("IPX_DEBUG_FORMS", None)
    A, Hz, c, b, lb, kw = box_schur_nine_windows()
    N = A.shape[1]
    Ad = dv.DeviceCSR.from_scipy(A)
    Z, _, Y = projector.projections(Ad)
    solver = Z.projector.solver
    assert type(solver).__name__ == "BoxSchurNormalSolver"
    geo = (ctypes.c_int32 * 2)()
    assert _hip.load().ipx_banded_decoupled_geometry(ctypes.c_void_p(solver.inner.handle), geo)
    assert geo[1] >= 9
    Hd = dv.DeviceCSR.from_scipy(Hz)
    assert cg_fused.supports(Hd, Z, Y)
    before = cg_fused.STATS["calls"]
    x, info = cg_fused.projected_cg(Hd, dv.DVec.from_host(c), Z, Y, dv.DVec.from_host(b),
                                    lb=dv.DVec.from_host(lb), **kw)
    assert cg_fused.STATS["calls"] == before + 1
    x1 = x.to_host()
    Zo, _, Yo = oracle.projections(A)
    xo, io = oracle.projected_cg(Hz, c, Zo, Yo, b, lb=lb, ub=np.full(N, np.inf), **kw)
    do = np.max(np.abs(x1 - xo)) / max(np.max(np.abs(xo)), 1e-300)
    print("windows %d, vs oracle %.3g (%d iterations)" % (geo[1], do, io["niter"]))
    assert (io["niter"], io["stop_cond"], io["hits_boundary"]) == \
        (info["niter"], info["stop_cond"], info["hits_boundary"])
    assert do <= 1e-9
