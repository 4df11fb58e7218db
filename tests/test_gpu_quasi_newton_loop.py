"""A low-rank (quasi-Newton) Hessian term inside the device CG loop's own launches
(ipx_cg_args.LR_*) against the same Hessian applied by the host between iterations
(``IPX_DEBUG_FORMS=no-lowrank-loop``): the banded three-launch form, the box-Schur form, the
dense-Jacobian form and a Hessian that is the low-rank term plus a diagonal."""
import numpy as np
import pytest
import scipy.sparse as sps

import ipsolver
from banded_setup import BandedInstance
from test_gpu_quasi_newton import _pairs, _device_sequence

pytestmark = pytest.mark.gpu


def _term(n, kind=0, memory=5, seed=0):
    strategy = ipsolver.LBFGS(memory) if kind == 0 else ipsolver.LSR1(memory)
    mem, _ = _device_sequence(strategy, _pairs(kind, n, memory + 2, np.random.default_rng(seed)),
                              n, [])
    return mem.term


def _both(monkeypatch, H, c, Z, Y, b, operator_loop=True, **kw):
    """the solve with the term in the loop, then with the host applying it (operator_loop: in
    the device loop's operator form; else -- dense Jacobians, whose device loop takes no
    operator Hessian -- on the statement-by-statement driver)"""
    from ipsolver import cg_fused, qp
    ops = cg_fused.STATS["operator_calls"]
    calls = cg_fused.STATS["calls"]
    monkeypatch.delenv("IPX_DEBUG_FORMS", raising=False)
    x, info = qp.projected_cg(H, c, Z, Y, b, **kw)
    assert cg_fused.STATS["calls"] == calls + 1                 # the device loop ran
    assert cg_fused.STATS["operator_calls"] == ops              # ... with no host products
    monkeypatch.setenv("IPX_DEBUG_FORMS", "no-lowrank-loop")
    x_op, info_op = qp.projected_cg(H, c, Z, Y, b, **kw)
    if operator_loop:
        assert cg_fused.STATS["operator_calls"] > ops            # the operator form
    else:
        assert cg_fused.STATS["calls"] == calls + 1              # the host-driven loop
    monkeypatch.delenv("IPX_DEBUG_FORMS")
    x, x_op = x.to_host(), x_op.to_host()
    assert info == info_op
    assert np.max(np.abs(x - x_op)) <= 1e-12 * max(1.0, np.max(np.abs(x_op)))
    return x, info


@pytest.mark.parametrize("kind", [0, 1])
def test_banded_three_launch_form(monkeypatch, kind):
    from ipsolver import backend_hip, cg_fused, projector
    from ipsolver.device import DeviceCSR, DVec
    inst = BandedInstance(20000, 2000)
    A = DeviceCSR.from_scipy(inst.A)
    Z, _, Y = projector.projections(A)
    H = backend_hip.hessian_operator([inst.H, _term(inst.n, kind)], inst.n, None)
    assert H.lowrank is not None and cg_fused._loop_parts(H)[0] is not None
    L = cg_fused._Loop(H, Z.projector, None, None)
    assert L.args.LR_W and L.args.H_hmax > 0 and L.args.r_next     # step2 + H.p, step1 + A.r fused
    for kw in (dict(tol=1e-12, max_iter=60), dict(trust_radius=1e-2, max_iter=60)):
        _both(monkeypatch, H, inst.c, Z, Y, np.zeros(inst.m), **kw)


def test_lowrank_plus_diagonal_without_csr(monkeypatch):
    from ipsolver import backend_hip, cg_fused, projector
    from ipsolver.device import DeviceCSR, DVec
    inst = BandedInstance(20000, 2000)
    A = DeviceCSR.from_scipy(inst.A)
    Z, _, Y = projector.projections(A)
    d = DVec.from_host(np.random.default_rng(4).uniform(0.5, 2.0, inst.n))
    H = backend_hip.hessian_operator([_term(inst.n, 0, 4), d], inst.n, None)
    Hc, Hd, LR = cg_fused._loop_parts(H)
    assert Hc is None and Hd is not None and LR is not None
    _both(monkeypatch, H, inst.c, Z, Y, np.zeros(inst.m), tol=1e-12,
          max_iter=60)


def test_box_schur_form_in_z_space(monkeypatch):
    from ipsolver import backend_hip, projector
    from ipsolver.device import DeviceCSR, DVec
    n, m = 6000, 600
    rng = np.random.default_rng(n)
    inst = BandedInstance(n, m)
    s = rng.uniform(0.05, 2.0, m + 2 * n)
    I = sps.eye(n, format="csr")
    A = sps.bmat([[inst.A, sps.diags(s[:m]), None, None],
                  [-I, None, sps.diags(s[m:m + n]), None],
                  [I, None, None, sps.diags(s[m + n:])]], format="csr")
    A.sort_indices()
    Z, _, Y = projector.projections(DeviceCSR.from_scipy(A))
    assert type(Z.projector.solver).__name__ == "BoxSchurNormalSolver"
    slack = DVec.from_host(rng.uniform(0.1, 2.0, m + 2 * n))
    H = backend_hip.hessian_operator([inst.H, _term(n, 1, 6)], n, slack)
    N = A.shape[1]
    assert H.shape == (N, N) and H.lowrank.shape[0] == n
    c = rng.standard_normal(N)
    _both(monkeypatch, H, c, Z, Y, np.zeros(A.shape[0]), tol=1e-12, max_iter=40)


def test_dense_jacobian_form(monkeypatch):
    from ipsolver import backend_hip, projector
    from ipsolver.dense import DeviceDense
    rng = np.random.default_rng(3)
    m, n = 60, 400
    A = rng.standard_normal((m, n))
    Hh = sps.diags([np.full(n - 1, 0.1), np.full(n, 2.0), np.full(n - 1, 0.1)], [-1, 0, 1])
    H = backend_hip.hessian_operator([sps.csr_matrix(Hh), _term(n, 0, 3)], n, None)
    Z, _, Y = projector.projections(DeviceDense.from_host(A))
    c = rng.standard_normal(n)
    b = A @ rng.standard_normal(n) * 0.01
    _both(monkeypatch, H, c, Z, Y, b, operator_loop=False, tol=1e-13)


def test_sqp_chain_and_resident_form_refuse_the_term():
    from ipsolver import backend_hip, cg_fused
    n = 2000
    H = backend_hip.hessian_operator([sps.identity(n, format="csr") * 2.0, _term(n)], n, None)
    assert cg_fused._hessian_parts(H) is None          # (what sqp_chain / the sharded loop take)
    assert cg_fused._loop_parts(H) is not None
