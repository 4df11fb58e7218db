"""The four entry points of csrc/sqp.hip called on their own, on constructed operands, against
the plain numpy transcriptions of tests/sqp_chain_cases.py.

Exact tier (disjoint-row A, integer data: every sum exact in any order): vectors and block
entries are compared for equality of every double (``==`` with NaN == NaN: bit for bit up to the
sign of a zero).  The projector's solve IS exact on the disjoint-row A (asserted once per problem
against the numpy value, ``test_the_solve_is_exact_on_disjoint_rows``), so the Newton-point and
dogleg cases stay in this tier.  Tolerance tier (tests/banded_setup.BandedInstance): references
in extended precision from the device's own input vectors, bound ``cc.sum_tolerance``.

Every call: the block is filled with 64 sentinels first and every entry the stage does not own
(``cc.OWNED``) keeps its bits; the published host copy equals the device block; output vectors
are pre-filled with NaN.  One case per entry point runs the quiet form (``host_block`` NULL).

Shapes (``cc.SHAPES``): one / two / few / slots / capped workgroups of the vector kernels; g = 258
with gm = 257 leaves no room for rows of four, so ``slots`` has rows 4 e_i + e_{i+1} (judge, model,
refresh: exact all the same) and ``slots_n`` the same n with disjoint rows (normal step, dogleg).
"""
import functools
import math

import numpy as np
import pytest
import torch

import sqp_chain_cases as cc

pytestmark = pytest.mark.gpu

COUNTS = {"exact": 0, "tolerance": 0}
NAN = float("nan")


# ---- comparisons --------------------------------------------------------------------------------
def exact(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    COUNTS["exact"] += 1
    if got.shape != want.shape or not np.array_equal(got, want, equal_nan=True):
        bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want)))) \
            if got.shape == want.shape else []
        raise AssertionError("%s: %d entries differ, first at %s: %r != %r" % (
            what, len(bad), bad[:4], got.ravel()[bad[:4]] if len(bad) else got.shape,
            want.ravel()[bad[:4]] if len(bad) else want.shape))


def close(got, want, tol, what):
    COUNTS["tolerance"] += 1
    err = np.max(np.abs(np.asarray(got, dtype=np.longdouble) - np.asarray(want, dtype=np.longdouble)))
    print("%s: error %.3e, bound %.3e" % (what, float(err), float(np.max(tol))))
    assert np.all(np.abs(np.asarray(got, dtype=np.longdouble) - want) <= tol), (what, float(err))


def within_ulps(got, want, ulps, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = np.maximum(np.abs(got), np.abs(want))
    close(got, want, ulps * np.spacing(scale), what)


def host(t):
    return t.cpu().numpy()


def put(t, a):
    t.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)))


# ---- problems and rigs (built once per module) --------------------------------------------------
class DeviceProblem:
    def __init__(self, pb, A, H):
        import ipsolver.device as dv
        import ipsolver.projector as proj
        self.pb = pb
        self.A, self.H = dv.DeviceCSR.from_scipy(A), dv.DeviceCSR.from_scipy(H)
        self.Z, _, self.Y = proj.projections(self.A)
        self.P = self.Z.projector
        torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def exact_problem(name):
    pb = cc.ExactProblem(name)
    return DeviceProblem(pb, pb.A, pb.H)


class TolProblem:
    """A BandedInstance with the attributes of cc.ExactProblem the rig reads."""

    def __init__(self, name):
        inst = cc.tolerance_instance(name)
        self.inst, self.n, self.m = inst, inst.n, inst.m
        self.A, self.H = inst.A.tocsr(), inst.H.tocsr()
        self.x, self.c, self.b = inst.x, inst.c, inst.b
        self.scale = np.ones(inst.n)


@functools.lru_cache(maxsize=None)
def tol_problem(name):
    pb = TolProblem(name)
    return DeviceProblem(pb, pb.A, pb.H)


_RIGS = {}


class Rig:
    """A StepChain bound to a problem's operands and a CG loop object, as sqp.ChainStages.propose
    binds them."""

    def __init__(self, dp, has_lb, has_ub, scale):
        import ipsolver.cg_fused as cg_fused
        import ipsolver.device as dv
        from ipsolver import sqp_chain as sc
        pb = dp.pb
        self.dp, self.pb = dp, pb
        self.chain = sc.StepChain(pb.n, pb.m, has_lb, has_ub)
        self.L, self.key = cg_fused._loop_for(dp.H, dp.P, self.chain.lbt_vec, self.chain.ubt_vec)
        assert sc.StepChain.fits(dp.A, dp.Z, dp.Y, dp.H, None, ())
        self.x, self.c, self.b = (dv.DVec.from_host(v) for v in (pb.x, pb.c, pb.b))
        self.lb = dv.DVec.from_host(np.full(pb.n, -64.0)) if has_lb else None
        self.ub = dv.DVec.from_host(np.full(pb.n, 64.0)) if has_ub else None
        self.scale = dv.DVec.from_host(pb.scale) if scale else None
        self.x_next = torch.full((pb.n,), NAN, dtype=torch.float64, device=self.x.t.device)
        self.chain.bind(self.L, dp.P, self.x, self.c, self.b, self.lb, self.ub, self.scale,
                        self.x_next)
        self.L.args.no_radius = 0

    def nan_outputs(self, keep_dn=False):
        ch = self.chain
        for t in (ch.ct, ch.d, ch.Hd, ch.Ad, self.x_next) + (() if keep_dn else (ch.dn,)):
            t.fill_(NAN)


def rig(dp, has_lb=True, has_ub=True, scale=True):
    key = (id(dp), has_lb, has_ub, scale)
    if key not in _RIGS:
        _RIGS[key] = Rig(dp, has_lb, has_ub, scale)
    return _RIGS[key]


@pytest.fixture(scope="module", autouse=True)
def _release_loops():
    yield
    import ipsolver.cg_fused as cg_fused
    torch.cuda.synchronize()
    for r in _RIGS.values():
        cg_fused._release(r.L, r.key)
    _RIGS.clear()
    print("\nexact-tier assertions: %(exact)d, tolerance-tier assertions: %(tolerance)d" % COUNTS)


@pytest.fixture(autouse=True)
def _stop_at_a_device_error():
    """A HIP error is sticky: nothing more is started on the device behind one."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device error, no further GPU work: %s" % e, returncode=3)


# ---- the block around a call ---------------------------------------------------------------------
_HOST_SENTINEL = 7.0e6


def arm(chain, inputs):
    """Sentinels into the device block (``inputs`` over them) and into the host copy."""
    q0 = cc.sentinels().copy()
    for k, v in inputs.items():
        q0[k] = v
    put(chain.q, q0)
    for i in range(cc.SIZE):
        chain.block[i] = _HOST_SENTINEL + i
    torch.cuda.synchronize()
    return q0


class quiet_form:
    """``host_block`` NULL for the calls inside."""

    def __init__(self, chain):
        self.chain = chain

    def __enter__(self):
        self.keep = self.chain.args.host_block
        self.chain.args.host_block = None

    def __exit__(self, *exc):
        self.chain.args.host_block = self.keep


def check_block(chain, q0, owned, expect, what, quiet=False):
    torch.cuda.synchronize()
    q = host(chain.q)
    blk = np.array(chain.block[:])
    if quiet:
        exact(blk, _HOST_SENTINEL + np.arange(cc.SIZE), what + ": host block of the quiet form")
    else:
        exact(blk, q, what + ": published block")
    others = [i for i in range(cc.SIZE) if i not in owned]
    exact(q[others], q0[others], what + ": entries of other stages %s" % (others,))
    assert set(expect) <= set(owned), sorted(set(expect) - set(owned))
    for k in sorted(expect):
        exact(q[k], expect[k], what + ": block[%d]" % k)
    return q


def publish_carries(chain, q_before, what):
    """A (non-quiet) verdict behind a quiet chain: its publish carries the quiet chain's entries."""
    import ipsolver.device as dv
    b_next = dv.DVec.from_host(np.ones(chain.m))
    chain.judge(b_next, 0.0)
    torch.cuda.synchronize()
    blk, q = np.array(chain.block[:]), host(chain.q)
    exact(blk, q, what + ": the next publish")
    keep = [i for i in range(cc.SIZE) if i not in cc.OWNED["judge"]]
    exact(blk[keep], q_before[keep], what + ": the next publish carries the quiet chain's entries")


# ---- ipx_sqp_judge -----------------------------------------------------------------------------
class JudgeRig:
    def __init__(self, m):
        import ipsolver.device as dv
        from ipsolver import sqp_chain as sc
        self.chain = ch = sc.StepChain(m + 1, m, False, False)
        g, gm = cc.grid_for(m + 1), cc.grid_for(m)
        ch.part = torch.zeros(64 * g + 16 * gm + 4096, dtype=torch.float64, device=ch.q.device)
        ch.args.part = ch.part.data_ptr()
        self.b_next = dv.DVec.from_host(cc.judge_b_next(m))


@functools.lru_cache(maxsize=None)
def judge_rig(m):
    return JudgeRig(m)


def _judge_expect(q_in, b_next, f_next):
    """The transcription, and ratio_host / radius_host on the same block with the exact norm."""
    from ipsolver import sqp_chain as sc
    out = cc.stage_judge(q_in, b_next, f_next)
    blk = sc.new_block()
    for k, v in q_in.items():
        blk[k] = v
    blk[cc.F_NEXT], blk[cc.NORM_B_NEXT] = f_next, out[cc.NORM_B_NEXT]
    sc.ratio_host(blk)
    if blk[cc.SOC] == 0.0:
        sc.radius_host(blk)
    else:
        blk[cc.ACCEPT] = 0.0
    for k in cc.OWNED["judge"]:
        exact(blk[k], out[k], "host decision functions against the statements: block[%d]" % k)
    return out


@pytest.mark.parametrize("m", cc.JUDGE_M)
def test_judge_every_rung(m):
    r = judge_rig(m)
    b_next = host(r.b_next.t)
    for rung in cc.JUDGE_RUNGS:
        q_in, f_next = cc.judge_case(rung, b_next)
        out = _judge_expect(q_in, b_next, f_next)
        assert cc.judge_rung_reached(out, q_in) == rung
        q0 = arm(r.chain, q_in)
        r.chain.judge(r.b_next, f_next)
        check_block(r.chain, q0, cc.OWNED["judge"], out, "judge m=%d %s" % (m, rung))


@pytest.mark.parametrize("m", [1, 1250, 262200])
def test_judge_device_scalar_nan_and_quiet_form(m):
    r = judge_rig(m)
    b_next = host(r.b_next.t)
    q_in, f_next = cc.judge_case("intermediary", b_next)
    out = _judge_expect(q_in, b_next, f_next)
    # f_next as a device scalar (the by-value argument is then ignored)
    q0 = arm(r.chain, q_in)
    f_dev = torch.tensor([f_next], dtype=torch.float64, device=r.chain.q.device)
    r.chain.judge(r.b_next, f_dev)
    check_block(r.chain, q0, cc.OWNED["judge"], out, "judge m=%d f_next_dev" % m)
    # the quiet form
    q0 = arm(r.chain, q_in)
    with quiet_form(r.chain):
        r.chain.judge(r.b_next, f_next)
    q = check_block(r.chain, q0, cc.OWNED["judge"], out, "judge m=%d quiet" % m, quiet=True)
    publish_carries(r.chain, q, "judge m=%d quiet" % m)
    # a NaN in b_next: NaN norm, NaN ratio, no acceptance, the penalty taken back
    import ipsolver.device as dv
    bad = b_next.copy()
    bad[m // 2] = NAN
    out = cc.stage_judge(q_in, bad, f_next)
    assert math.isnan(out[cc.NORM_B_NEXT]) and math.isnan(out[cc.RATIO]) and out[cc.ACCEPT] == 0.0
    assert out[cc.RADIUS] == q_in[cc.RADIUS] and out[cc.PENALTY] == q_in[cc.PREV_PENALTY]
    q0 = arm(r.chain, q_in)
    r.chain.judge(dv.DVec.from_host(bad), f_next)
    check_block(r.chain, q0, cc.OWNED["judge"], out, "judge m=%d NaN" % m)


# ---- ipx_sqp_model -----------------------------------------------------------------------------
BOUNDS = {"none": (False, False), "lbt": (True, False), "ubt": (False, True), "both": (True, True)}
MODEL_HOST_CASES = [(s, b) for s in ("one", "two", "few") for b in BOUNDS] + \
    [("slots", "both"), ("capped", "both")]


def _state_sentinels(L):
    s = 3.0e5 + 0.5 * np.arange(L.state.numel())
    put(L.state, s)
    return s


def _load_model_operands(r, dn, dt, lbt, ubt, p=None):
    ch = r.chain
    put(ch.dn, dn)
    put(r.L.x, dt)
    if p is not None:
        put(r.L.p, p)
    if ch.lbt is not None:
        put(ch.lbt, lbt)
    if ch.ubt is not None:
        put(ch.ubt, ubt)


def _check_model_vectors(r, st, what):
    ch = r.chain
    for name, t in (("d", ch.d), ("x_next", r.x_next), ("Hd", ch.Hd), ("Ad", ch.Ad)):
        exact(host(t), st[name], "%s: %s" % (what, name))


@pytest.mark.parametrize("shape,bounds", MODEL_HOST_CASES)
def test_model_after_a_host_driven_cg(shape, bounds):
    dp = exact_problem(shape)
    pb = dp.pb
    has_lb, has_ub = BOUNDS[bounds]
    r = rig(dp, has_lb, has_ub, scale=bounds in ("both", "lbt"))
    lbt, ubt = (pb.lbt if has_lb else None), (pb.ubt if has_ub else None)
    scale = pb.scale if r.scale is not None else None
    penalty, f, norm_b = 2.0, 3.5, 9.0
    what = "model host_cg %s %s" % (shape, bounds)
    for form in ("plain", "quiet") if bounds == "both" else ("plain",):
        r.nan_outputs(keep_dn=True)
        _load_model_operands(r, pb.dn, pb.dt, lbt, ubt)
        state = _state_sentinels(r.L)
        st = cc.stage_model(pb, pb.dn, pb.dt, lbt, ubt, scale, penalty, f, norm_b)
        expect = dict(st["block"])
        expect.update({cc.CG + i: state[i] for i in range(16)})
        assert expect[cc.PRIME_STEPS] == 0.0
        q0 = arm(r.chain, {})
        if form == "quiet":
            with quiet_form(r.chain):
                r.chain.model(penalty, f, norm_b, host_cg=True)
        else:
            r.chain.model(penalty, f, norm_b, host_cg=True)
        q = check_block(r.chain, q0, cc.OWNED["model_host_cg"], expect, what, quiet=form == "quiet")
        _check_model_vectors(r, st, what)
        exact(host(r.L.x), pb.dt, what + ": dt untouched")
        if form == "quiet":
            publish_carries(r.chain, q, what)


@pytest.mark.parametrize("shape", ["one", "few"])
def test_model_counts_a_nan_of_dt_as_outside(shape):
    dp = exact_problem(shape)
    pb = dp.pb
    r = rig(dp, True, True, scale=True)
    dt = pb.dt.copy()
    j = int(np.flatnonzero((pb.lbt < pb.dt) & (pb.dt < pb.ubt))[0])
    dt[j] = NAN
    r.nan_outputs(keep_dn=True)
    _load_model_operands(r, pb.dn, dt, pb.lbt, pb.ubt)
    state = _state_sentinels(r.L)
    st = cc.stage_model(pb, pb.dn, dt, pb.lbt, pb.ubt, pb.scale, 2.0, 3.5, 9.0)
    assert st["block"][cc.X_OUTSIDE] == len(pb.outside) + 1
    assert all(math.isnan(st["block"][k]) for k in (cc.NORM_D, cc.NORM_DT, cc.CD, cc.HDD))
    expect = dict(st["block"])
    expect.update({cc.CG + i: state[i] for i in range(16)})
    q0 = arm(r.chain, {})
    r.chain.model(2.0, 3.5, 9.0, host_cg=True)
    check_block(r.chain, q0, cc.OWNED["model_host_cg"], expect, "model NaN in dt " + shape)
    _check_model_vectors(r, st, "model NaN in dt " + shape)


@pytest.mark.parametrize("case", cc.EXIT_CASES)
@pytest.mark.parametrize("shape", ["one", "few", "slots"])
def test_model_boundary_exits(shape, case):
    """host_cg = 0 on a hand-written loop state.  tau within 4 ulp of the oracle's
    box_sphere_intersections; dt, d and x_next for equality with numpy's clip(dt + tau p) taken
    with the DEVICE's tau (-ffp-contract=off makes that well defined); the sums, which are exact
    only where tau is a power of two, within ``cc.sum_tolerance`` of the references taken from
    the device's own d and dt."""
    import ipsolver.cg_fused as cg_fused
    dp = exact_problem(shape)
    pb = dp.pb
    r = rig(dp, True, True, scale=True)
    stop, alpha, radius, z, p, lbt, ubt = cc.exit_case(pb, case)
    what = "model exit %s %s" % (shape, case)
    r.nan_outputs(keep_dn=True)
    _load_model_operands(r, pb.dn, z, lbt, ubt, p)
    state = _state_sentinels(r.L)
    state[[cg_fused.ST_STOP, cg_fused.ST_ALPHA, cg_fused.ST_RADIUS]] = stop, alpha, radius
    put(r.L.state, state)
    steps = (1.0, 0.0) if case.endswith("2") else (1.0, 1.0)
    red = np.zeros(24)
    red[16:18] = steps
    put(r.chain.red, red)
    ex = cc.stage_exit(stop, alpha, radius, z, p, lbt, ubt)
    q0 = arm(r.chain, {})
    quiet = case == "box-2"
    if quiet:
        with quiet_form(r.chain):
            r.chain.model(2.0, 3.5, 9.0, host_cg=False)
    else:
        r.chain.model(2.0, 3.5, 9.0, host_cg=False)
    expect = {cc.EXIT_DONE: ex["done"], cc.PRIME_STEPS: steps[0] + steps[1], cc.F: 3.5,
              cc.NORM_B: 9.0}
    expect.update({cc.CG + i: state[i] for i in range(16)})
    if ex["tau"] == 0.0:
        expect[cc.EXIT_TAU] = 0.0
    q = check_block(r.chain, q0, cc.OWNED["model"], expect, what, quiet=quiet)
    tau = q[cc.EXIT_TAU]
    within_ulps(tau, ex["tau"], 4, what + ": tau")
    dt_new = cc.clip_step(z, tau, p, lbt, ubt) if ex["done"] else z
    exact(host(r.L.x), dt_new, what + ": dt")
    if case.startswith("plain"):
        assert cc.inside_count(dt_new, lbt, ubt) == 1        # (neither moved nor clipped)
    if case.startswith("miss"):
        assert not np.array_equal(dt_new, z)                 # (clipped all the same)
    st = cc.stage_model(pb, pb.dn, dt_new, lbt, ubt, pb.scale, 2.0, 3.5, 9.0, steps[0] + steps[1])
    _check_model_vectors(r, st, what)
    exact(q[cc.X_OUTSIDE], st["block"][cc.X_OUTSIDE], what + ": X_OUTSIDE")
    for k in (cc.NORM_D, cc.NORM_DT, cc.LIN):
        tol = cc.sum_tolerance(st["terms"][k], pb.n)
        close(q[k] ** 2, math.fsum(st["terms"][k]), tol + 4 * np.spacing(q[k] ** 2),
              what + ": block[%d]^2" % k)
    for k in (cc.CD, cc.HDD):
        close(q[k], math.fsum(st["terms"][k]), cc.sum_tolerance(st["terms"][k], pb.n),
              what + ": block[%d]" % k)
    exact([q[i] for i in (cc.QMODEL, cc.VPRED, cc.PREV_PENALTY, cc.PENALTY, cc.PRED, cc.MERIT)],
          [cc.model_entries(q[cc.HDD], q[cc.CD], q[cc.LIN], 9.0, 2.0, 3.5)[i] for i in
           (cc.QMODEL, cc.VPRED, cc.PREV_PENALTY, cc.PENALTY, cc.PRED, cc.MERIT)],
          what + ": the model on the device's sums")
    if quiet:
        publish_carries(r.chain, q, what)


# ---- ipx_sqp_front -----------------------------------------------------------------------------
def _front(r, have_dn, with_dogleg, radius, penalty, f, norm_b, quiet=False):
    ch = r.chain
    put(ch.red, np.zeros(24))
    r.L.x.fill_(NAN)
    r.L.v.fill_(NAN)
    if ch.lbt is not None:
        ch.lbt.fill_(NAN)
    if ch.ubt is not None:
        ch.ubt.fill_(NAN)
    r.nan_outputs(keep_dn=bool(have_dn))
    _state_sentinels(r.L)
    ch.expect_steps = False
    ch.front(have_dn, with_dogleg, radius, penalty, f, norm_b, r.dp.P.norm_A, 0, quiet=quiet)
    torch.cuda.synchronize()


def _set_bounds(r, lb, ub):
    if r.lb is not None:
        put(r.lb.t, lb)
    if r.ub is not None:
        put(r.ub.t, ub)


def _check_front_rest(r, dn, lb, ub, q, what, exact_sums=True):
    """What follows the normal step: c_t, the shifted bounds, a zero dt, the model on d = dn, the
    copy of the loop's state."""
    pb, ch = r.pb, r.chain
    lb = lb if r.lb is not None else None
    ub = ub if r.ub is not None else None
    ctb = cc.stage_ct_bounds(pb.H, pb.c, dn, lb, ub)
    if ch.lbt is not None:
        exact(host(ch.lbt), ctb["lbt"], what + ": lbt")
    if ch.ubt is not None:
        exact(host(ch.ubt), ctb["ubt"], what + ": ubt")
    exact(host(r.L.x), np.zeros(pb.n), what + ": dt = 0")
    exact(q[cc.CG:cc.CG + 16], host(r.L.state)[:16], what + ": copy of the loop's state")
    exact([q[cc.EXIT_TAU], q[cc.EXIT_DONE], q[cc.PRIME_STEPS]], [0.0, 0.0, 0.0], what + ": no exit")
    scale = pb.scale if r.scale is not None else None
    st = cc.stage_model(pb, dn, np.zeros(pb.n), ctb["lbt"], ctb["ubt"], scale, 2.0, 3.5, 9.0)
    exact(host(ch.d), st["d"], what + ": d")
    exact(host(r.x_next), st["x_next"], what + ": x_next")
    if exact_sums:
        exact(host(ch.ct), ctb["ct"], what + ": ct")
        exact(host(ch.Hd), st["Hd"], what + ": Hd")
        exact(host(ch.Ad), st["Ad"], what + ": Ad")
        for k, v in st["block"].items():
            exact(q[k], v, what + ": block[%d]" % k)


@pytest.mark.parametrize("name", sorted(k for k, v in cc.SHAPES.items() if v[2] == "disjoint"))
def test_the_solve_is_exact_on_disjoint_rows(name):
    """(A A')^-1 b with A A' = diag(4, 16, ...): the device's solve gives b_i / 4, b_i / 16."""
    import ipsolver.device as dv
    dp = exact_problem(name)
    v = dp.P.solver.solve(dv.DVec.from_host(dp.pb.b))
    torch.cuda.synchronize()
    exact(v.to_host(), dp.pb.newton()[0], "solve on disjoint rows, " + name)
    w = dp.A.dot(dv.DVec.from_host(dp.pb.c))
    v = dp.P.solver.solve(w)
    torch.cuda.synchronize()
    exact(v.to_host(), (dp.pb.A @ dp.pb.c) / dp.pb.aat_diag(), "product and solve, " + name)


@pytest.mark.parametrize("bounds", ["both", "lbt", "ubt"])
@pytest.mark.parametrize("shape", ["one", "two", "few", "slots_n"])
def test_front_with_a_given_normal_step(shape, bounds):
    dp = exact_problem(shape)
    pb = dp.pb
    has_lb, has_ub = BOUNDS[bounds]
    r = rig(dp, has_lb, has_ub, scale=bounds == "both")
    rng = np.random.default_rng(9)
    lb, ub = -64.0 + rng.integers(0, 8, pb.n), 64.0 - rng.integers(0, 8, pb.n)
    _set_bounds(r, lb, ub)
    norm_dn = float(np.sqrt(np.sum(pb.dn ** 2)))
    for radius, quiet in ((2.0 * norm_dn, False), (0.5 * norm_dn, False)) + \
            (((2.0 * norm_dn, True),) if bounds == "both" else ()):
        what = "front given dn %s %s radius %g%s" % (shape, bounds, radius, " quiet" * quiet)
        put(r.chain.dn, pb.dn)
        expect = cc.stage_given(pb.dn, radius)
        assert math.isnan(expect[cc.RADIUS_T]) == (radius < norm_dn)
        q0 = arm(r.chain, {})
        _front(r, 1, 0, radius, 2.0, 3.5, 9.0, quiet=quiet)
        q = check_block(r.chain, q0, cc.OWNED["front"], expect, what, quiet=quiet)
        exact(host(r.chain.dn), pb.dn, what + ": dn untouched")
        _check_front_rest(r, pb.dn, lb, ub, q, what)
        if quiet:
            publish_carries(r.chain, q, what)


@pytest.mark.parametrize("shape", ["one", "few"])
def test_front_hands_the_priming_its_radius_and_sums(shape):
    """The loop's r, p and state behind the front equal a separate ipx_cg_prime call on the c_t
    and RADIUS_T the front produced."""
    import ipsolver.cg_fused as cg_fused
    import ipsolver.device as dv
    from ipsolver import _hip
    dp = exact_problem(shape)
    pb = dp.pb
    r = rig(dp, True, True, scale=True)
    _set_bounds(r, pb.lb, pb.ub)
    put(r.chain.dn, pb.dn)
    radius = 4.0 * float(np.sqrt(np.sum(pb.dn ** 2)))
    arm(r.chain, {})
    _front(r, 1, 0, radius, 2.0, 3.5, 9.0)
    q = host(r.chain.q)
    twin = cg_fused._Loop(dp.H, dp.P, r.chain.lbt_vec, r.chain.ubt_vec, arm=False)
    for t in (twin.x, twin.r, twin.p, twin.Hp):
        t.fill_(NAN)
    _state_sentinels(twin)
    red = torch.zeros(24, dtype=torch.float64, device=twin.x.device)
    pat = dp.A.pattern
    _hip.call("ipx_cg_prime", twin.ref(), dv._p(pat.tiles), pat.ntiles, dv._p(r.chain.ct), None,
              dv._p(red), dv._p(dv.ctx().ws), NAN, float(q[cc.RADIUS_T]), float(dp.P.orth_tol),
              float(dp.P.norm_A), float(dp.P.CANCELLATION), 0, 0, dv.stream_ptr())
    torch.cuda.synchronize()
    for name in ("x", "r", "p", "Hp", "state"):
        exact(host(getattr(r.L, name)), host(getattr(twin, name)), "priming %s: %s" % (shape, name))
    assert host(twin.state)[cg_fused.ST_RADIUS] == q[cc.RADIUS_T]


@pytest.mark.parametrize("case", list(cc.NEWTON_CASES))
@pytest.mark.parametrize("shape", ["one", "two", "few", "slots_n"])
def test_front_newton_point(shape, case):
    import ipsolver.device as dv
    dp = exact_problem(shape)
    pb = dp.pb
    r = rig(dp, True, True, scale=True)
    radius, lb, ub = cc.newton_case(pb, case)
    _set_bounds(r, lb, ub)
    v_ref, dn = pb.newton()
    expect = cc.stage_newton(dn, lb, ub, radius)
    assert expect[cc.NORMAL_KIND] == cc.NEWTON_CASES[case]
    what = "front newton %s %s" % (shape, case)
    quiet = case == "accepted"
    q0 = arm(r.chain, {})
    _front(r, 0, 0, radius, 2.0, 3.5, 9.0, quiet=quiet)
    q = check_block(r.chain, q0, cc.OWNED["front"], expect, what, quiet=quiet)
    # (the priming behind the normal step solves into the same v: the solve's operands and
    # buffers are held through dn = -A'v, against a separate solve and product)
    v_sep = dp.P.solver.solve(r.b)
    dn_sep = dp.A.T.dot(v_sep)
    torch.cuda.synchronize()
    exact(v_sep.to_host(), v_ref, what + ": the separate solve")
    exact(host(r.chain.dn), -dn_sep.to_host(), what + ": dn against a separate solve and product")
    exact(host(r.chain.dn), dn, what + ": dn")
    _check_front_rest(r, dn, lb, ub, q, what)
    if quiet:
        publish_carries(r.chain, q, what)


@pytest.mark.parametrize("case", list(cc.DOGLEG_CASES))
@pytest.mark.parametrize("shape", ["one", "few", "slots_n"])
def test_front_dogleg(shape, case):
    dp = exact_problem(shape)
    pb = dp.pb
    r = rig(dp, True, True, scale=True)
    radius, lb, ub = cc.dogleg_case(pb, case)
    _set_bounds(r, lb, ub)
    _, newton = pb.newton()
    nw = cc.stage_newton(newton, lb, ub, radius)
    what = "front dogleg %s %s" % (shape, case)
    q0 = arm(r.chain, {})
    _front(r, 0, 1, radius, 2.0, 3.5, 9.0)
    if case == "stands":
        # every dogleg launch a no-op: the vectors it borrows hold what the rest of the chain
        # writes, SQ_DOGLEG.. keep their sentinels
        assert nw[cc.NORMAL_KIND] == 1.0
        q = check_block(r.chain, q0, cc.OWNED["front"], nw, what)
        exact(host(r.chain.dn), newton, what + ": dn")
        _check_front_rest(r, newton, lb, ub, q, what)
        return
    dg = cc.stage_dogleg(pb, pb.b, lb, ub, radius)
    assert dg["branch"] == cc.DOGLEG_CASES[case] and nw[cc.NORMAL_KIND] == 0.0
    blk = dg["block"]
    expect = {cc.NVIOL: nw[cc.NVIOL], cc.NORMAL_KIND: 2.0, cc.RADIUS: radius,
              cc.DOGLEG: -0.125, cc.DOGLEG + 1: blk[cc.DOGLEG + 1], cc.DOGLEG + 4: blk[cc.DOGLEG + 4]}
    q = check_block(r.chain, q0, cc.OWNED["front_dogleg"], expect, what)
    within_ulps(q[cc.DOGLEG + 2], blk[cc.DOGLEG + 2], 4, what + ": alpha of x1")
    within_ulps(q[cc.DOGLEG + 3], blk[cc.DOGLEG + 3], 4, what + ": alpha of x2")
    dn = host(r.chain.dn)
    within_ulps(dn, dg["oracle_dn"], 4, what + ": dn against the oracle's modified_dogleg")
    # ||A x + b|| of the two candidates: the 4 ulp of the alphas reach a row's value b_i (1 - t)
    # amplified by t / (1 - t) <= 4 on these cases, the square doubles it
    rel = 2.0 ** -53 * (2 * cc.depth(pb.m) + 64)
    close(q[cc.DOGLEG + 5], dg["r1"], rel * dg["r1"], what + ": ||A x1 + b||")
    close(q[cc.DOGLEG + 6], dg["r2"], rel * dg["r2"], what + ": ||A x2 + b||")
    nn = math.fsum(dn * dn)
    close(q[cc.NORM_DN] ** 2, nn, cc.sum_tolerance(dn * dn, pb.n) + 4 * np.spacing(nn),
          what + ": NORM_DN^2")
    with np.errstate(invalid="ignore"):
        exact(q[cc.RADIUS_T], np.sqrt(np.float64(radius * radius - q[cc.NORM_DN] * q[cc.NORM_DN])),
              what + ": RADIUS_T from the device's NORM_DN")
    _check_front_rest(r, dn, lb, ub, q, what, exact_sums=dg["branch"][1] == "tie")


@pytest.mark.parametrize("case", ["accepted", "ball", "box"])
@pytest.mark.parametrize("shape", ["one", "two"])
def test_front_newton_point_on_real_data(shape, case):
    """Tolerance tier: dn against a separate solve and product (equality; the chain's own v is
    overwritten by the priming behind it), and against -A'v in extended precision from that
    solve's v; the decision (taken at a margin of 1e-6 at least) and the counts from the device's
    dn."""
    dp = tol_problem(shape)
    pb = dp.pb
    r = rig(dp, True, True, scale=False)
    radius, lb, ub, kind = cc.tolerance_newton_case(pb.inst, case)
    _set_bounds(r, lb, ub)
    what = "front newton (real data) %s %s" % (shape, case)
    q0 = arm(r.chain, {})
    _front(r, 0, 0, radius, 2.0, 3.5, 9.0)
    q = check_block(r.chain, q0, cc.OWNED["front"], {cc.NORMAL_KIND: kind, cc.RADIUS: radius}, what)
    v_sep = dp.P.solver.solve(r.b)
    dn_sep = dp.A.T.dot(v_sep)
    torch.cuda.synchronize()
    v = v_sep.to_host()
    dn = host(r.chain.dn)
    exact(dn, -dn_sep.to_host(), what + ": dn against a separate solve and product")
    At = pb.A.T.tocsr()
    ld = np.longdouble
    ref = -np.array([np.sum(At.data[s:e].astype(ld) * v[At.indices[s:e]].astype(ld))
                     for s, e in zip(At.indptr[:-1], At.indptr[1:])], dtype=ld)
    mag = np.abs(At) @ np.abs(v)
    rowlen = np.diff(At.indptr)
    close(dn, ref, (rowlen + 1) * 2.0 ** -53 * mag, what + ": dn = -A'v")
    assert min(cc.newton_margins(dn, radius, lb, ub)) >= cc.MARGIN
    exact(q[cc.NVIOL], cc.inside_count(dn, cc.BOX_FACTOR * lb, cc.BOX_FACTOR * ub), what + ": NVIOL")
    nn = math.fsum(dn * dn)
    close(q[cc.NORM_DN] ** 2, nn, cc.sum_tolerance(dn * dn, pb.n) + 4 * np.spacing(nn),
          what + ": NORM_DN^2")
    with np.errstate(invalid="ignore"):
        exact(q[cc.RADIUS_T], np.sqrt(np.float64(radius * radius - q[cc.NORM_DN] * q[cc.NORM_DN])),
              what + ": RADIUS_T from the device's NORM_DN")
    exact(host(r.chain.lbt), lb - dn, what + ": lbt")
    exact(host(r.chain.ubt), ub - dn, what + ": ubt")
    exact(host(r.L.x), np.zeros(pb.n), what + ": the loop's x zeroed")
    exact(host(r.chain.d), dn + 0.0, what + ": d")


# ---- ipx_sqp_refresh ---------------------------------------------------------------------------
class RefreshRig:
    def __init__(self, dp):
        import ipsolver.device as dv
        from ipsolver import sqp_chain as sc
        pb = dp.pb
        self.dp = dp
        self.chain = sc.StepChain(pb.n, pb.m, False, False)
        self.c, self.b = dv.DVec.from_host(pb.c), dv.DVec.from_host(pb.b)
        self.v_out = torch.full((pb.m,), NAN, dtype=torch.float64, device=self.c.t.device)
        self.chain.bind_refresh(dp.P, self.c, self.b, self.v_out)


@functools.lru_cache(maxsize=None)
def refresh_rig(tier, shape):
    return RefreshRig(exact_problem(shape) if tier == "exact" else tol_problem(shape))


REFRESH_CASES = [("tol", "one"), ("tol", "two"), ("tol", "few"), ("exact", "one"), ("exact", "few"),
                 ("exact", "slots"), ("exact", "capped")]


@pytest.mark.parametrize("tier,shape", REFRESH_CASES)
def test_refresh(tier, shape):
    import ipsolver.device as dv
    r = refresh_rig(tier, shape)
    dp, pb, ch = r.dp, r.dp.pb, r.chain
    what = "refresh %s %s" % (tier, shape)
    w = dp.A.dot(r.c)
    v_sep = dp.P.solver.solve(w).to_host()
    A = pb.A.tocsr()
    At = A.T.tocsr()
    rowlen = np.diff(At.indptr)
    for form in ("norm-A", "plain", "quiet"):
        r.v_out.fill_(NAN)
        verdict = form != "plain"
        put(ch.verdict, [5.0, 0.0])
        q0 = arm(ch, {})
        norm_part = dp.P.norm_partials() if form == "norm-A" else None
        if form == "quiet":
            with quiet_form(ch):
                ch.refresh(norm_part, verdict)
        else:
            ch.refresh(norm_part, verdict)
        owned = cc.OWNED["refresh_norm_A" if form == "norm-A" else "refresh"]
        expect = {cc.FACTOR_BAD: 5.0 if verdict else 0.0, cc.VIOL: float(np.max(np.abs(pb.b)))}
        if tier == "exact":
            expect[cc.NORM_B] = float(np.sqrt(np.sum(pb.b ** 2)))
            if form == "norm-A":
                expect[cc.NORM_A2] = float(np.sum(A.data ** 2))
        q = check_block(ch, q0, owned, expect, what + " " + form, quiet=form == "quiet")
        v_out = host(r.v_out)
        exact(v_out, -v_sep, what + ": v_out against the negated separate product and solve")
        if tier == "exact":
            # c + A'v: rows of A' hold at most two entries here, so the row sum is one rounding
            # whatever its order, and the transcription on the device's v gives the same doubles
            ref = cc.stage_refresh(A, pb.c, pb.b, -v_out)
            assert int(rowlen.max()) <= 2
            exact(q[cc.OPT], ref["block"][cc.OPT], what + ": OPT")
            if pb.kind == "disjoint":
                exact(v_out, -((A @ pb.c) / pb.aat_diag()), what + ": v_out")
        else:
            ld = np.longdouble
            ct = pb.c.astype(ld) + np.array(
                [np.sum(At.data[s:e].astype(ld) * v_out[At.indices[s:e]].astype(ld))
                 for s, e in zip(At.indptr[:-1], At.indptr[1:])], dtype=ld)
            mag = np.abs(pb.c) + np.abs(At) @ np.abs(v_out)
            row_tol = (rowlen + 2) * 2.0 ** -53 * mag
            close(q[cc.OPT], np.max(np.abs(ct)), float(np.max(row_tol)), what + ": OPT")
            nb = math.fsum(pb.b ** 2)
            close(q[cc.NORM_B] ** 2, nb, cc.sum_tolerance(pb.b ** 2, pb.m) + 4 * np.spacing(nb),
                  what + ": NORM_B^2")
            if form == "norm-A":
                nnz = len(A.data)
                d = -(-nnz // (dv._reduce_grid(nnz) * 256)) + 8 + 12
                close(q[cc.NORM_A2], math.fsum(A.data ** 2), cc.sum_tolerance(A.data ** 2, d=d),
                      what + ": NORM_A2")
        if form == "quiet":
            publish_carries(ch, q, what)
