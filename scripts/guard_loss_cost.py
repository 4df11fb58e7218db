"""What the radius guard (csrc/cg.hip, ipx_cg_args.rguard) costs a call that loses it, and how
loose its bound is, on the benchmark's problem (n = 1e6, m = 1e5, max_iter = 40):

  1. one call at radius 1e300 in batches of one iteration: X_k, Q_k against ||x_k||, ||p_k||
     (float64 norms on the device) -- the looseness X / ||x|| along the trajectory;
  2. a radius just above ||x_40||: the iterates never reach it, the bound does at a known
     iteration k, the call runs all 40 iterations -- k_rguard_sums, one step2 + H.p in the
     carried form and one state read more than the exact form (IPX_DEBUG_FORMS=no-radius-guard);
     median of 20 calls each, alternating.

    python3 scripts/guard_loss_cost.py > guard_loss_cost.txt
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ip-nonlinear-solver_amd"))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from ipsolver import cg_fused, device as dv, projector, qp
from ipsolver.operators import DeviceHessian
from ipsolver.synthetic import CenteredBandedNLP

n, K = 1000000, 40
m = n // 10
prob = CenteredBandedNLP(n, m, seed=0)
x = prob.x0
v = 0.1 * np.random.default_rng(7).standard_normal(m)
A = dv.DeviceCSR.from_scipy(prob.constr_jac(x))
H = DeviceHessian(n, csr=dv.DeviceCSR.from_scipy(prob.hess(x)),
                  diag=dv.DVec.from_host(prob.kappa * prob.Wt.dot(v)))
c = dv.DVec.from_host(prob.grad(x))
b = dv.DVec.zeros(m)
Z, LS, Y = projector.projections(A)


def call(radius, form="", **kw):
    os.environ["IPX_DEBUG_FORMS"] = form
    cg_fused._GUARD_LOST.clear()
    before = dict(cg_fused.STATS)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if kw:      # (batch: the device loop's own argument)
        xs, info = cg_fused.projected_cg(H, c, Z, Y, b, trust_radius=radius, tol=0, max_iter=K,
                                         b_zero=True, **kw)
    else:
        xs, info = qp.projected_cg(H, c, Z, Y, b, trust_radius=radius, tol=0, max_iter=K)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return xs, info, dt, {k: cg_fused.STATS[k] - before[k] for k in before}


# 1. the trajectory of the bounds
seen = []


def watch(L, last):
    X, Q, _ = L.rguard.tolist()
    seen.append((last[1], X, Q, float(torch.linalg.vector_norm(L.x)),
                 float(torch.linalg.vector_norm(L.p)), int(L.args.radius_guard)))


cg_fused._WATCH_BATCHES.append(watch)
call(1e300, batch=1)
cg_fused._WATCH_BATCHES.clear()
print("it      X          ||x||      X/||x||    Q          ||p||      Q/||p||   armed")
for it, X, Q, nx, npn, armed in seen:
    print("%3d  %.6e  %.6e  %8.4f  %.6e  %.6e  %8.4f  %d"
          % (it, X, nx, X / nx if nx else float("nan"), Q, npn, Q / npn if npn else float("nan"),
             armed))
print("largest X/||x|| %.4f, largest Q/||p|| %.4f over %d iterations"
      % (max(s[1] / s[3] for s in seen if s[3]), max(s[2] / s[4] for s in seen if s[4]), len(seen)))

# 2. a radius the iterates stay inside and the bound does not
radius = seen[-1][3] * (1.0 + 1e-6)
lost_at = next(s[0] for s in seen if s[1] >= radius)     # T of iteration lost_at - 1 is X here
for form in ("", "no-radius-guard"):
    for _ in range(3):
        call(radius, form)
times = {"": [], "no-radius-guard": []}
for _ in range(20):
    for form in times:
        xs, info, dt, d = call(radius, form)
        assert info["niter"] == K and info["stop_cond"] == 1, info
        assert d["guard_lost"] == (1 if form == "" else 0), d
        times[form].append(dt)
g, e = statistics.median(times[""]), statistics.median(times["no-radius-guard"])
print("radius %.6e (||x_40|| (1 + 1e-6)): the bound reaches it in iteration %d of %d"
      % (radius, lost_at - 1, K))
print("call that loses the guard: median of 20 %.1f us (min %.1f, max %.1f)"
      % (g * 1e6, min(times[""]) * 1e6, max(times[""]) * 1e6))
print("same call, no-radius-guard: median of 20 %.1f us (min %.1f, max %.1f)"
      % (e * 1e6, min(times["no-radius-guard"]) * 1e6, max(times["no-radius-guard"]) * 1e6))
print("price of losing the guard: %+.1f us per call (%+.2f %%)" % ((g - e) * 1e6, (g / e - 1) * 100))
# and what a call that keeps it gains over the same 40 iterations
times = {"": [], "no-radius-guard": []}
for _ in range(20):
    for form in times:
        xs, info, dt, d = call(1e300, form)
        assert d["guard_lost"] == 0
        times[form].append(dt)
g, e = statistics.median(times[""]), statistics.median(times["no-radius-guard"])
print("call that keeps the guard (radius 1e300): median of 20 %.1f us, no-radius-guard %.1f us: "
      "%+.1f us per call" % (g * 1e6, e * 1e6, (g - e) * 1e6))
