"""Single ``projected_cg`` calls out of the REFERENCE's barrier runs on the config-5 style
problem (box on every variable + nonlinear inequalities), from the first barrier parameter to
the last (mu <= 1e-6: slacks of active bounds ~1e-8, the regime the cancellation-free box-Schur
formulas of csrc/boxschur.hip exist for).  tests/golden/make_golden.py --late-barrier recorded
what the reference passed to ``projected_cg`` (equality_constrained_sqp.py:125-132, assembled
by tr_interior_point.py:141-241) and what it returned; here the product solves the same
subproblems through its own path -- augmented Jacobian, z-space Hessian operator, box-Schur
projections, device-resident loop -- on one GPU and row-sharded over two processes.

What "the same answer" means here.  Late in the barrier run the gradient of the subproblem lies
almost entirely in the row space of the Jacobian: ``Z c`` cancels 6-8 digits of ``c``
(|c| = 2.8, |Z c| = 1e-8 at mu = 1e-8), so ANY implementation -- the reference's included --
has the projection to ``eps |c| / |Z c|`` only, and hundreds of CG iterations amplify that.
The generator therefore also measured how well the reference's own answer is determined:
(a) its ``Z c`` against the exact projection (augmented system refined in long double):
2e-16 at mu = 0.1, 4e-9 at mu = 1e-8; (b) its ``projected_cg`` result when every component of
``c`` moves by ONE unit in the last place (four seeded sign patterns): identical counts and
1e-15 early, 271..272 iterations and 3e-5 in x at mu = 2.6e-7.  The assertions below hold the
product to exactly that: integers exact wherever the reference's own count does not move under
one ulp (within its spread over the four perturbed runs + 0.1 % of the count where it does),
vectors to 1e-10 or TWICE the reference's own one-ulp sensitivity, the projection NO FURTHER
from the exact one than the reference's own (or 4 eps) and within 16 ulp of its INPUT's size.
(Round 3 allowed ten times the reference's figures: the normal equations form ``c - A'v`` by
one subtraction that cancels six digits and were 7-9x further from the exact projection than
the reference at mu = 1e-4 ... 1e-6; ``null_space`` now adds one correction step on z itself
when that subtraction has cancelled more than ten bits -- projector.py -- and is 0.2x the
reference's distance there: scripts/late_barrier_margins.py prints the table.)"""
import os

import numpy as np
import pytest
import scipy.sparse as sps

from banded_setup import load_synthetic
from conftest import load_npz

pytestmark = pytest.mark.gpu

SIZES = {400: 6, 12000: 4}


def _gold(n):
    return load_npz("late_barrier_n%d" % n)


def _pieces(gold, j):
    """The data of call j as the reference's SQP held it."""
    n, m = (int(v) for v in gold["n"])
    g = lambda k: gold["c%d_%s" % (j, k)]
    sens, proj = g("sens"), g("proj")
    spread = int(np.max(np.abs(sens[:, 0] - g("info")[0])))
    return dict(n=n, m=m, x=g("x_vars"), s=g("s"), v_nl=g("v_nl"), Hs=g("Hs"), c=g("c"),
                lb=g("lb"), radius=float(g("radius")), mu=float(g("mu")), x_out=g("x"),
                info=[int(v) for v in g("info")], allvecs=g("allvecs"),
                stride=int(gold["stride"][0]), z_true=g("z_true"), ref_proj_err=float(proj[0]),
                # what one ulp in c does to the reference's own result: its iteration count's
                # spread over FOUR perturbed runs (a sample maximum) + 0.1 % of the count
                niter_slack=0 if spread == 0 else spread + int(np.ceil(0.001 * g("info")[0])),
                x_tol=max(1e-10, 2.0 * float(sens[:, 3].max())),
                it_tol=max(1e-10, 2.0 * float(sens[:, 4].max())))


def close_rel(a, b, tol):
    a, b = np.asarray(a), np.asarray(b)
    scale = max(np.max(np.abs(b)), 1e-300)
    err = np.max(np.abs(a - b)) / scale
    assert err <= tol, "relative deviation %.3e > %.1e" % (err, tol)
    return err


def _solve_single(d, return_all=False, projection_only=False):
    """The product's own assembly (backend_hip: augmented Jacobian with the slack entries,
    Hessian terms merged into one fused SpMV + diagonal) and solve."""
    from ipsolver import backend_hip as xp
    from ipsolver import cg_fused
    from ipsolver.device import DVec
    n, m = d["n"], d["m"]
    n_ineq = m + 2 * n
    prob = load_synthetic().CenteredBandedNLP(n, m, eps=1.0)
    eye = sps.identity(n, format="csr")
    J_ineq = sps.vstack([prob.constr_jac(d["x"]), -eye, eye], format="csr")
    A = xp.augmented_jacobian(sps.csr_matrix((0, n)), J_ineq, DVec.from_host(d["s"]), n, 0, n_ineq)
    H = xp.hessian_operator([prob.hess(d["x"]), prob.constr_hess(d["x"], d["v_nl"])], n,
                            DVec.from_host(d["Hs"]))
    Z, LS, Y = xp.projections(A)
    assert type(Z.projector.solver).__name__ == "BoxSchurNormalSolver"
    assert cg_fused.supports(H, Z, Y)
    if projection_only:
        return Z.dot(DVec.from_host(d["c"])).to_host()
    N = n + n_ineq
    calls = cg_fused.STATS["calls"]
    x, info = xp.projected_cg(H, DVec.from_host(d["c"]), Z, Y, DVec.zeros(n_ineq), d["radius"],
                              DVec.from_host(d["lb"]), DVec.full(N, np.inf),
                              **({"return_all": True} if return_all else {}))
    if not return_all:
        assert cg_fused.STATS["calls"] == calls + 1, "device-resident loop not taken"
    return x, info


@pytest.mark.parametrize("n", sorted(SIZES))
def test_late_barrier_subproblems_single_gpu(n):
    """Every recorded call, the last ones included (criteria: module docstring)."""
    gold = _gold(n)
    assert len(gold["picks"]) == SIZES[n]
    for j in range(SIZES[n]):
        d = _pieces(gold, j)
        # the projection against the exact one: as close as the reference's own
        z = _solve_single(d, projection_only=True)
        zerr = np.max(np.abs(z - d["z_true"]))
        assert zerr <= max(4 * 2.2204e-16, d["ref_proj_err"]) * np.max(np.abs(d["z_true"])), \
            (j, zerr / np.max(np.abs(d["z_true"])), d["ref_proj_err"])
        assert zerr <= 16 * 2.2204e-16 * np.max(np.abs(d["c"]))
        # the device-resident loop
        x, info = _solve_single(d)
        assert [info["stop_cond"], int(info["hits_boundary"])] == d["info"][1:], (j, info, d["info"])
        assert abs(info["niter"] - d["info"][0]) <= d["niter_slack"], \
            (j, d["mu"], info["niter"], d["info"][0], d["niter_slack"])
        xerr = close_rel(x.to_host(), d["x_out"], d["x_tol"])
        # the general driver (same kernels, host-side control flow) for the iterates
        xg, ig = _solve_single(d, return_all=True)
        assert [ig["stop_cond"], int(ig["hits_boundary"])] == d["info"][1:]
        assert abs(ig["niter"] - d["info"][0]) <= d["niter_slack"]
        st, iterr = d["stride"], 0.0
        for k, want in enumerate(d["allvecs"][:len(ig["allvecs"])]):
            iterr = max(iterr, close_rel(ig["allvecs"][k].to_host()[::st], want, d["it_tol"]))
        print("late barrier n=%d call %d mu=%.1e: niter %d (reference %d, slack %d); x dev %.1e "
              "(bound %.1e); first iterates %.1e (bound %.1e); projection error %.1e "
              "(reference's own %.1e)" % (n, j, d["mu"], info["niter"], d["info"][0],
                                          d["niter_slack"], xerr, d["x_tol"], iterr, d["it_tol"],
                                          zerr / np.max(np.abs(d["z_true"])), d["ref_proj_err"]))


def _sharded_worker(rank, world, port, out_path):
    import sys
    import torch
    import torch.distributed as dist
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "ip-nonlinear-solver_amd"), os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from ipsolver import sharded, qp
        n = 12000
        gold = _gold(n)
        out = {}
        for j in range(SIZES[n]):
            d = _pieces(gold, j)
            m = d["m"]
            prob = load_synthetic().CenteredBandedNLP(n, m, eps=1.0)
            J = prob.constr_jac(d["x"]).tocsr()
            lay = sharded.ShardLayout(J.indptr, J.indices, J.shape, world, rank)
            sh = sharded.Sharding(lay, sharded.ShardComm(), sharded.HipOps())
            xp = sharded.ShardedBackend(sh)
            sh.register(xp.INEQ)
            sh.register(xp.Z)
            n_ineq = m + 2 * n
            # the distributed pieces as barrier.py assembles them on the sharded backend
            Jn = sharded.BoxInequalityJacobian(sharded.ShardCSR.from_global(sh, J))
            A = xp.augmented_jacobian(None, Jn, sh.from_global(d["s"], xp.INEQ), n, 0, n_ineq)
            Hx = sharded.ShardHessian.from_global(sh, prob.hess(d["x"]),
                                                  prob.kappa * prob.Wt.dot(d["v_nl"]))
            H = xp.hessian_operator(Hx, n, sh.from_global(d["Hs"], xp.INEQ))
            Z, LS, Y = xp.projections(A)
            calls = sharded.STATS["fused_calls"]
            x, info = qp.projected_cg(H, sh.from_global(d["c"], xp.Z), Z, Y, sh.zeros(xp.INEQ),
                                      d["radius"], sh.from_global(d["lb"], xp.Z), None)
            assert sharded.STATS["fused_calls"] == calls + 1, "device-resident sharded loop not taken"
            out["x%d" % j] = x.to_host()
            out["info%d" % j] = np.array([info["niter"], info["stop_cond"],
                                          int(info["hits_boundary"])])
        out["transport"] = np.array([float(sh.transport == "ipc"),
                                     sh.mailbox().fused_launches() if sh.mailbox() else 0,
                                     sh.comm.stats["ipc_iterations"]])
        if rank == 0:
            np.savez(out_path, **out)
    finally:
        dist.destroy_process_group()


def test_late_barrier_subproblems_two_ranks(tmp_path):
    """The same recorded calls (n = 12000) on the row-sharded backend: two processes, the
    distributed z = [x; s_nl; s_lb; s_ub], box-Schur projections on every rank, the
    device-resident loop with its reductions and halo exchange through the peer mailboxes --
    held to the reference's results by the same criteria."""
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    path = str(tmp_path / "late.npz")
    mp.spawn(_sharded_worker, args=(2, port, path), nprocs=2, join=True)
    got = np.load(path)
    assert got["transport"][0] == 1.0
    # the four-segment z-space loop did its collectives in the prologues of its own kernels
    # (k_cg_step1_box / k_cg_step2_hp, PEER forms: 5 launches per iteration, no pack kernels)
    assert got["transport"][1] == 2 * got["transport"][2] > 0
    gold = _gold(12000)
    for j in range(SIZES[12000]):
        d = _pieces(gold, j)
        info = [int(v) for v in got["info%d" % j]]
        assert info[1:] == d["info"][1:], (j, info, d["info"])
        assert abs(info[0] - d["info"][0]) <= d["niter_slack"], (j, info, d["info"])
        err = close_rel(got["x%d" % j], d["x_out"], d["x_tol"])
        print("late barrier, 2 ranks, call %d mu=%.1e: niter %d (reference %d), x dev %.1e "
              "(bound %.1e)" % (j, d["mu"], info[0], d["info"][0], err, d["x_tol"]))
