"""The launch sequence of the projected-CG loop's host code (csrc/cg.hip), form by form, pinned
through the library's own host counter ``ipx_launch_count``.

One short public ``projected_cg`` call per form leaves a bound, primed loop object (the one the
call parks in ``cg_fused._POOL``; caught where it is released, because a dense-Jacobian loop is
not pooled).  With stop code 9 in its state block -- the code priming uses for "the launches do
nothing" -- every kernel returns at once, so the entry points can be called in any order:
``ipx_cg_iterate(0, 1)`` and ``(0, 6)`` give the launches per iteration (difference / 5) and the
constant per batch, ``ipx_cg_resume``, ``ipx_cg_step2_hp``, ``ipx_cg_hp`` and ``ipx_cg_save_pb``
one count each.  ``ipx_cg_step2_hp`` on a block that does not enable the fused kernel must
return IPX_EINVAL and launch nothing.

The counts are facts about the host code alone; EXPECTED holds them as measured at the commit
named there, before the loop drivers were rewritten around one loop plan.  The one count the
project documents -- DESIGN.md §3: "One CG iteration on the benchmark = 3 launches", the banded
fused loop with an infinite or carried radius -- is asserted on its own, not from the table.

Shapes: (2000, 200) has 3 row tiles of H and one slice of carried partials; (50000, 5000) has
74 row tiles, two slices, no array long enough to be compacted (tests/test_gpu_cg_radius_sums.py).
The box-Schur instance is the smallest of tests/test_gpu_qp.py's
(test_box_schur_projection_without_matrix_rows: n, m = 6000, 600, every variable bounded), the
dense one has the row and column counts of test_gpu_dense_inequality.py's smallest structured
Gram case (7 + 30 rows, 301 + 30 columns), the low-rank ones are test_gpu_quasi_newton_loop.py's
dense-Jacobian case (its smallest) and, for the term behind the fused step2 + H.p kernel, its
banded case.  m = 0: the public call keeps such problems off the device loop, so the block is
the (2000, 200) one with m set to 0 on a copy -- what a C caller would pass.
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sps

from banded_setup import BandedInstance

pytestmark = pytest.mark.gpu

IPX_EINVAL = -1


@functools.lru_cache(maxsize=None)
def banded(n, m):
    import ipsolver.device as dv
    import ipsolver.projector as proj
    inst = BandedInstance(n, m)
    A = dv.DeviceCSR.from_scipy(inst.A)
    H = dv.DeviceCSR.from_scipy(inst.H)
    Z, _, Y = proj.projections(A)
    return dict(H=H, c=inst.c, Z=Z, Y=Y, b=np.zeros(m), kw=dict(trust_radius=1e300))


@functools.lru_cache(maxsize=None)
def box_schur():
    import ipsolver.device as dv
    import ipsolver.projector as proj
    n, m = 6000, 600
    rng = np.random.default_rng(7)
    inst = BandedInstance(n, m)
    I = sps.eye(n, format="csr")
    s = rng.uniform(1e-6, 2.0, m + 2 * n)
    A = sps.bmat([[inst.A, sps.diags(s[:m]), None, None],
                  [-I, None, sps.diags(s[m:m + n]), None],
                  [I, None, None, sps.diags(s[m + n:])]], format="csr")
    A.sort_indices()
    N, M = A.shape[1], A.shape[0]
    Z, _, Y = proj.projections(dv.DeviceCSR.from_scipy(A))
    assert type(Z.projector.solver).__name__ == "BoxSchurNormalSolver"
    Hz = sps.block_diag([inst.H, sps.diags(rng.uniform(0.5, 2.0, N - n))], format="csr")
    lb = np.concatenate((np.full(n, -np.inf), np.full(N - n, -0.995)))
    return dict(H=dv.DeviceCSR.from_scipy(Hz), c=rng.standard_normal(N), Z=Z, Y=Y, b=np.zeros(M),
                kw=dict(trust_radius=5.0, lb=lb))


@functools.lru_cache(maxsize=None)
def dense():
    import ipsolver.projector as proj
    from ipsolver.dense import DeviceDense
    rng = np.random.default_rng(3)
    m, n = 37, 331
    A = rng.standard_normal((m, n))
    G = rng.standard_normal((n, n))
    H = DeviceDense.from_host(G @ G.T / n + np.eye(n))
    Z, _, Y = proj.projections(DeviceDense.from_host(A))
    return dict(H=H, c=rng.standard_normal(n), Z=Z, Y=Y, b=np.zeros(m), kw=dict(trust_radius=10.0))


def _term(n, kind, memory, seed=0):
    import ipsolver
    from test_gpu_quasi_newton import _pairs, _device_sequence
    strategy = ipsolver.LBFGS(memory) if kind == 0 else ipsolver.LSR1(memory)
    mem, _ = _device_sequence(strategy, _pairs(kind, n, memory + 2, np.random.default_rng(seed)),
                              n, [])
    return mem.term


@functools.lru_cache(maxsize=None)
def lowrank_dense():
    from ipsolver import backend_hip, projector
    from ipsolver.dense import DeviceDense
    rng = np.random.default_rng(3)
    m, n = 60, 400
    A = rng.standard_normal((m, n))
    Hh = sps.diags([np.full(n - 1, 0.1), np.full(n, 2.0), np.full(n - 1, 0.1)], [-1, 0, 1])
    H = backend_hip.hessian_operator([sps.csr_matrix(Hh), _term(n, 0, 3)], n, None)
    Z, _, Y = projector.projections(DeviceDense.from_host(A))
    return dict(H=H, c=rng.standard_normal(n), Z=Z, Y=Y, b=np.zeros(m), kw=dict(trust_radius=10.0))


@functools.lru_cache(maxsize=None)
def lowrank_banded():
    from ipsolver import backend_hip
    base = banded(20000, 2000)
    inst = BandedInstance(20000, 2000)
    H = backend_hip.hessian_operator([inst.H, _term(inst.n, 0, 5)], inst.n, None)
    return dict(base, H=H)


def _fused(a):
    return bool(a.r_next) and a.A_span > 0 and a.H_hmax > 0 and bool(a.At_vown) and not a.resident


# name -> (IPX_DEBUG_FORMS, problem, changes to a copy of the argument block, what the block
# the public call built must look like for the case to be the one it is named after)
FORMS = {
    "carried-2000": ("no-resident", lambda: banded(2000, 200), {},
                     lambda a: _fused(a) and bool(a.xsums) and a.H_ntiles == 3),
    "carried-50000": ("no-resident", lambda: banded(50000, 5000), {},
                      lambda a: _fused(a) and bool(a.xsums) and a.H_ntiles == 74),
    "reading-2000": ("no-resident,read-xn2", lambda: banded(2000, 200), {},
                     lambda a: _fused(a) and not a.xsums),
    "reading-2000-no-radius": ("no-resident,read-xn2", lambda: banded(2000, 200),
                               {"no_radius": 1}, lambda a: _fused(a) and not a.xsums),
    "resident-2000": ("", lambda: banded(2000, 200), {}, lambda a: a.resident == 1),
    "separate-2000": ("no-fuse", lambda: banded(2000, 200), {},
                      lambda a: not a.r_next and not a.pb and not a.At_vown and not a.resident),
    "box-schur-6000": ("", box_schur, {}, lambda a: a.solver_kind == 1 and bool(a.lb)),
    "dense-331": ("", dense, {}, lambda a: a.solver_kind == 2 and not a.H_rowptr),
    "m0-2000": ("no-resident", lambda: banded(2000, 200), {"m": 0}, _fused),
    "lowrank-dense-400": ("", lowrank_dense, {},
                          lambda a: a.solver_kind == 2 and bool(a.LR_W) and bool(a.H_rowptr)),
    "lowrank-banded-20000": ("no-resident", lowrank_banded, {},
                             lambda a: _fused(a) and bool(a.LR_W)),
}

# Measured with this module's ``measure`` at commit 2beb1a4 ("Projected CG: form the radius test
# from sums carried by step2+H.p"), the parent of the loop-plan rewrite:
#   per_iteration, per_batch, resume, step2_hp (None: IPX_EINVAL, nothing launched), hp, save_pb
EXPECTED = {
    "carried-2000": (3, 0, 3, 1, 2, 1),
    "carried-50000": (3, 0, 3, 1, 2, 1),
    "reading-2000": (3, 0, 3, 1, 2, 1),
    "reading-2000-no-radius": (3, 0, 3, 1, 2, 1),
    "resident-2000": (0, 2, 3, 1, 2, 1),
    "separate-2000": (6, 0, 2, None, 1, 0),
    "box-schur-6000": (3, 0, 3, 1, 2, 1),
    "dense-331": (7, 0, 2, None, 1, 0),
    "m0-2000": (2, 1, 3, 1, 2, 1),
    "lowrank-dense-400": (9, 0, 4, None, 3, 0),
    "lowrank-banded-20000": (5, 0, 5, 3, 4, 1),
}

# the banded fused loop with an infinite or carried radius is 3 launches
THREE_LAUNCHES = ("carried-2000", "carried-50000", "reading-2000-no-radius")


def loop_object(monkeypatch, name):
    """The loop object one short public call on the form's problem leaves behind."""
    import ipsolver.cg_fused as cg_fused
    import ipsolver.qp as qp
    env, problem = FORMS[name][:2]
    if env:
        monkeypatch.setenv("IPX_DEBUG_FORMS", env)
    else:
        monkeypatch.delenv("IPX_DEBUG_FORMS", raising=False)
    q = problem()
    caught = []
    real = cg_fused._release

    def release(L, key):
        caught.append(L)
        return real(L, key)

    monkeypatch.setattr(cg_fused, "_release", release)
    calls = cg_fused.STATS["calls"]
    qp.projected_cg(q["H"], q["c"], q["Z"], q["Y"], q["b"], tol=0, max_iter=3, **q["kw"])
    monkeypatch.setattr(cg_fused, "_release", real)
    assert cg_fused.STATS["calls"] == calls + 1 and caught      # the device loop ran
    L = caught[-1]
    if any(L is v for v in cg_fused._POOL.values()):
        assert L is next(reversed(cg_fused._POOL.values()))
    return L


def measure(monkeypatch, name):
    import torch
    import ipsolver.cg_fused as cg_fused
    import ipsolver.device as dv
    from ipsolver import _hip
    L = loop_object(monkeypatch, name)
    a = cg_fused.CgArgs.from_buffer_copy(L.args)
    assert FORMS[name][3](a), name
    for field, value in FORMS[name][2].items():
        setattr(a, field, value)
    a.xsums_carry = 0
    ref, st, lib = ctypes.byref(a), dv.stream_ptr(), _hip.load()
    saved = L.state.clone()
    L.state[cg_fused.ST_STOP] = 9.0
    torch.cuda.synchronize()

    def launches(fn, *args):
        before = int(lib.ipx_launch_count())
        rc = fn(ref, *args, st)
        return rc, int(lib.ipx_launch_count()) - before

    try:
        rc1, one = launches(lib.ipx_cg_iterate, 0, 1)
        rc6, six = launches(lib.ipx_cg_iterate, 0, 6)
        assert rc1 == 0 and rc6 == 0
        assert (six - one) % 5 == 0
        per_it = (six - one) // 5
        rc, resume = launches(lib.ipx_cg_resume, 0, 0)
        assert rc == 0
        rc, s2hp = launches(lib.ipx_cg_step2_hp, 0, 0)
        enabled = bool(a.pb) and a.H_hmax > 0 and not a.H_operator
        assert rc == (0 if enabled else IPX_EINVAL)
        if not enabled:
            assert s2hp == 0
            s2hp = None
        rc, hp = launches(lib.ipx_cg_hp)
        assert rc == 0
        rc, save_pb = launches(lib.ipx_cg_save_pb)
        assert rc == 0
        torch.cuda.synchronize()
        assert float(L.state[cg_fused.ST_STOP].item()) == 9.0      # nothing ran
    finally:
        L.state.copy_(saved)
        torch.cuda.synchronize()
    return (per_it, one - per_it, resume, s2hp, hp, save_pb)


@pytest.mark.parametrize("name", list(FORMS))
def test_launch_counts(monkeypatch, name):
    got = measure(monkeypatch, name)
    print(name, got)
    if name in THREE_LAUNCHES:
        assert got[0] == 3
    assert got == EXPECTED[name]
