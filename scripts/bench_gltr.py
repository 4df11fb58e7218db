"""Projected GLTR (csrc/gltr.hip, ipsolver/gltr.py) by the clock: the parts of one Lanczos step at
n = 1e6, m = 1e5 on the bench's banded problem with an indefinite Hessian, the tridiagonal
trust-region launch at k = 8, 64, 256, the recombination at k = 64, and the outer iterations /
Hessian products / wall time of solves with and without ``options={'subproblem': 'gltr'}``.
GPU times are HIP events around the launches of one call, medians of the repetitions with the
smallest and largest beside them; solves are host wall clock.
    python scripts/bench_gltr.py [--quick] > profiles/gltr_timings.txt"""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ip-nonlinear-solver_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import ipsolver
from ipsolver import _hip, device as dv, projector, qp, gltr
from ipsolver.operators import DeviceHessian
from ipsolver.synthetic import CenteredBandedNLP

QUICK = "--quick" in sys.argv
sync = torch.cuda.synchronize


def gpu_us(fn, reps=30, warm=5):
    """(median, min, max) in microseconds of the GPU time of fn()'s launches."""
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sync()
        a.record()
        fn()
        b.record()
        sync()
        out.append(1e3 * a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def fmt(t):
    return "%9.1f us (%.1f .. %.1f)" % t


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def lanczos_step_parts(n, m):
    print("== one Lanczos step by parts, n = %d, m = %d (bench problem, Hessian made indefinite)" % (n, m))
    prob = CenteredBandedNLP(n, m, seed=0)
    x = prob.x0
    v = 0.1 * np.random.default_rng(7).standard_normal(m)
    rng = np.random.default_rng(3)
    Hs = prob.hess(x)
    shift = np.where(rng.random(n) < 0.3, -2.0 * np.abs(Hs.diagonal()).mean(), 0.0)
    A = dv.DeviceCSR.from_scipy(prob.constr_jac(x))
    H = DeviceHessian(n, csr=dv.DeviceCSR.from_scipy(Hs),
                      diag=dv.DVec.from_host(prob.kappa * prob.Wt.dot(v) + shift))
    c = dv.DVec.from_host(prob.grad(x))
    Z, LS, Y = projector.projections(A)
    print("(A A')^-1 solver:", type(Z.projector.solver).__name__)
    lib = _hip.load()
    kmax = 64
    W = gltr._work(n, kmax)
    g = Z.dot(Z.dot(c))
    radius = 0.05 * dv.norm(g)
    st = dv.stream_ptr
    P = dv._p
    q0 = W.cols[0]

    def start():
        _hip.call("ipx_gltr_start", n, kmax, kmax, P(g.t), P(W.Q), P(W.state), P(W.part), radius,
                  0.0, st())
    start()
    print("H product                    ", fmt(gpu_us(lambda: H.dot(q0))))
    w = H.dot(q0)
    print("projection Z                 ", fmt(gpu_us(lambda: Z.dot(w))))
    print("ipx_gltr_start (2 launches)  ", fmt(gpu_us(start)))
    # a live step again and again at the same k: the state is put back between the timings
    start()
    saved = None
    for k in range(kmax):
        w = Z.dot(H.dot(W.cols[k]))
        if k in (0, 7, 31, 63):
            saved = (W.state.clone(), W.Q[(k + 1) * n:(k + 2) * n].clone())

            def step(k=k, w=w, saved=saved):
                W.state.copy_(saved[0])
                _hip.call("ipx_gltr_step", n, kmax, P(w.t), P(W.Q), P(W.state), P(W.part), st())

            def restore(saved=saved):
                W.state.copy_(saved[0])
            t_all, t_copy = gpu_us(step), gpu_us(restore)
            hdr = None
            W.state.copy_(saved[0])
        _hip.call("ipx_gltr_step", n, kmax, P(w.t), P(W.Q), P(W.state), P(W.part), st())
        if k in (0, 7, 31, 63):
            hdr = dv.read_doubles(W.state, 16)
            print("ipx_gltr_step at k = %2d (4 launches, minus the state copy %.1f us) %s   "
                  "case %d, path %d, rounds %d" % (k + 1, t_copy[0], fmt(tuple(t - t_copy[0] for t in t_all)),
                                                     hdr[9], hdr[11], hdr[12]))
    stopped = gpu_us(lambda: _hip.call("ipx_gltr_step", n, kmax, P(w.t), P(W.Q), P(W.state),
                                       P(W.part), st()))
    print("ipx_gltr_step behind the stop word (4 empty launches)", fmt(stopped))
    x = dv._empty(n)
    t = gpu_us(lambda: _hip.call("ipx_gltr_combine", n, kmax, P(W.Q), P(W.state), None, P(x), st()))
    k = int(dv.read_doubles(W.state, 16)[1])
    gb = 8.0 * (k + 1) * n / 1e9
    print("ipx_gltr_combine at k = %d  %s   %.3f GB -> %.2f TB/s (8 k n bytes at the 6.29 TB/s "
          "copy rate: %.1f us)" % (k, fmt(t), gb, gb / t[0] * 1e3, 8.0 * k * n / 6.29e12 * 1e6))
    # the whole call against projected_cg on the same inputs
    for name, fn in (("projected_gltr (default tol)", lambda: qp.projected_gltr(H, c, Z, Y, None, radius)),
                     ("projected_cg   (default tol)", lambda: qp.projected_cg(H, c, Z, Y, None, radius))):
        fn()
        sync()
        t0 = time.perf_counter()
        xx, info = fn()
        sync()
        t1 = time.perf_counter()
        Hx = H.dot(xx)
        print("%s  %8.1f us wall, %s, model value %.9e"
              % (name, 1e6 * (t1 - t0), {k: info[k] for k in ("niter", "stop_cond", "hits_boundary")},
                 0.5 * float(Hx.dot(xx)) + float(c.dot(xx))))


def tridiagonal_launch():
    print("== ipx_gltr_tridiag alone (one workgroup)")
    rng = np.random.default_rng(0)
    for k in (8, 64, 256):
        cases = {
            "interior": (np.full(k, 4.0), np.ones(k), 1.0, 100.0),
            "boundary": (rng.standard_normal(k), np.abs(rng.standard_normal(k)) + 0.01, 1.0, 1.0),
            "near-hard": (rng.standard_normal(k) * 10 - 3, np.abs(rng.standard_normal(k)) * 0.1 + 0.01,
                          0.5, 50.0),
        }
        for name, (d, o, g0, R) in cases.items():
            dd, od = dev(d), dev(o)
            out = torch.zeros(8 + k, dtype=torch.float64, device="cuda")
            t = gpu_us(lambda: _hip.call("ipx_gltr_tridiag", k, dd.data_ptr(), od.data_ptr(), g0, R,
                                         out.data_ptr(), dv.stream_ptr()))
            r = out[:6].tolist()
            print("k = %3d %-9s %s   case %d, path %d, rounds %d" % (k, name, fmt(t), r[3], r[4], r[5]))


def solves():
    print("== solves with and without options={'subproblem': 'gltr'}: outer iterations, Hessian "
          "products, wall seconds (second of two runs)")
    import gltr_cases, blocktri_cases as bc
    rows = []
    p = gltr_cases.e2e_problems()[0]
    cons = p.constraints(ipsolver)
    rows.append(("rosenbrock10 on 2 planes, exact Hessian", p.fun, p.x0, p.grad, lambda: p.hess, cons))
    rows.append(("rosenbrock10 on 2 planes, LSR1", p.fun, p.x0, p.grad, ipsolver.LSR1, cons))
    J, rhs, target = bc.staged_problem(d=6, c=2, stages=(30 if QUICK else 200))
    n = J.shape[1]
    x0 = np.zeros(n)
    fun = lambda x: float(np.sum(0.5 * (x - target) ** 2 + 1.5 * np.cos(2 * x)))
    grad = lambda x: (x - target) - 3.0 * np.sin(2 * x)
    cons = ipsolver.LinearConstraint(J, ("equals", rhs))
    rows.append(("staged d=6 c=2, n = %d, m = %d, 1/2|x-t|^2 + 1.5 sum cos 2x, LSR1" % (n, J.shape[0]),
                 fun, x0, grad, ipsolver.LSR1, cons))
    for name, f, x0, g, hess, cons in rows:
        for sub in ("steihaug", "gltr"):
            for _ in range(2):
                sync()
                t0 = time.perf_counter()
                res = ipsolver.minimize_constrained(f, x0, g, hess(), cons,
                                                    options={"subproblem": sub})
                sync()
                t1 = time.perf_counter()
            print("%-70s %-8s status %d, outer %4d, products %5d, f = %.10e, %.3f s%s"
                  % (name, sub, res.status, res.niter, res.cg_niter, res.fun, t1 - t0,
                     "" if sub == "steihaug" else ", gltr calls %d (%d on the boundary)"
                     % (res.gltr_calls, res.gltr_boundary_calls)))


if __name__ == "__main__":
    print(torch.cuda.get_device_name(0))
    tridiagonal_launch()
    lanczos_step_parts(100000 if QUICK else 1000000, 10000 if QUICK else 100000)
    solves()
