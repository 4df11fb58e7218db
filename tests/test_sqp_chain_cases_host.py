"""The cases of tests/sqp_chain_cases.py are what they claim, without a device: the exact tier's
sums are integers (times a fixed power of two) below 2^53 in any order, every named branch is
reached by the case named after it according to the oracle, the tolerance tier's decisions keep
their margin, the grids are the ones the shapes' names promise.  (Run with ``-s`` for the list of
branches and the cases that reach them.)"""
import functools

import numpy as np
import pytest

import sqp_chain_cases as cc

SMALL = ["one", "two", "few"]
DISJOINT = [k for k, v in cc.SHAPES.items() if v[2] == "disjoint"]


@functools.lru_cache(maxsize=None)
def problem(name):
    return cc.ExactProblem(name)


def test_block_layout_is_the_library_s():
    from ipsolver import _hip, sqp_chain as sc
    import ipsolver.cg_fused as cg_fused
    for name in ("RADIUS PENALTY F NORM_B NORM_DN RADIUS_T NORMAL_KIND NVIOL HDD CD LIN NORM_D NORM_DT "
                 "QMODEL VPRED PREV_PENALTY PRED MERIT F_NEXT NORM_B_NEXT ACTUAL RATIO SOC ACCEPT OPT "
                 "VIOL NORM_A2 FACTOR_BAD EXIT_TAU EXIT_DONE X_OUTSIDE PRIME_STEPS CG SIZE").split():
        assert getattr(cc, name) == getattr(sc, name), name
    assert (cc.TR_FACTOR, cc.BOX_FACTOR) == (sc.TR_FACTOR, sc.BOX_FACTOR)
    assert (cc.ST_RADIUS, cc.ST_ALPHA, cc.ST_STOP) == (cg_fused.ST_RADIUS, cg_fused.ST_ALPHA,
                                                       cg_fused.ST_STOP)
    assert _hip.load().ipx_sqp_block_size() == cc.SIZE
    assert len(set(cc.sentinels())) == cc.SIZE
    for owned in cc.OWNED.values():
        assert len(set(owned)) == len(owned) and all(0 <= i < cc.SIZE for i in owned)


@pytest.mark.parametrize("name", sorted(cc.SHAPES))
def test_grids_are_the_ones_the_names_promise(name):
    n, m, kind, grids = cc.SHAPES[name]
    assert (cc.grid_for(n), cc.grid_for(m)) == grids
    assert n - m >= 1 and (kind != "disjoint" or n >= 4 * m)
    if name == "two":
        assert n == 2 * 512 + 1                  # (one element in the vector kernels' third trip)
    if name == "capped":
        assert n > 1024 * 1024 and cc.depth(n) == 5 + 20
    if name in cc.TOL_SHAPES:
        assert cc.TOL_SHAPES[name] == (n, m)


def _assert_integer_sum(terms, what):
    """float64 sums in three orders against the integer sum of the terms x 2^12."""
    t = np.asarray(terms, dtype=np.float64)
    scaled = t * 4096.0
    ints = scaled.astype(np.int64)
    assert np.array_equal(ints.astype(np.float64), scaled), what
    total = int(np.sum(ints.astype(object))) if len(ints) < 10000 else int(np.sum(ints))
    assert int(np.sum(np.abs(ints))) < 2 ** 53, what
    rng = np.random.default_rng(3)
    for order in (t, t[::-1], t[rng.permutation(len(t))]):
        s = 0.0
        for chunk in np.array_split(order, 7):   # (numpy's pairwise order inside, ours across)
            s += float(np.sum(chunk))
        assert s * 4096.0 == total, what
        assert float(np.cumsum(order)[-1]) * 4096.0 == total, what


@pytest.mark.parametrize("name", sorted(cc.SHAPES))
def test_exact_tier_sums_are_integers_below_2_53(name):
    pb = problem(name)
    st = cc.stage_model(pb, pb.dn, pb.dt, pb.lbt, pb.ubt, pb.scale, 2.0, 3.0, 1.0)
    for key, terms in st["terms"].items():
        _assert_integer_sum(terms, ("model", key))
    _assert_integer_sum(pb.b_next ** 2, "b_next")
    _assert_integer_sum(pb.b ** 2, "b")
    _assert_integer_sum(pb.dn ** 2, "dn")
    _assert_integer_sum(pb.A.data ** 2, "A")
    assert np.array_equal(st["x_next"] * 16, np.round(st["x_next"] * 16))
    ct = cc.stage_ct_bounds(pb.H, pb.c, pb.dn, pb.lb, pb.ub)["ct"]
    assert np.array_equal(ct * 16, np.round(ct * 16))
    if pb.kind == "disjoint":
        S = (pb.A @ pb.A.T).tocsr()
        assert S.nnz == pb.m and np.array_equal(S.diagonal(), pb.aat_diag())
        assert np.sum(np.diff(pb.A.T.tocsr().indptr) == 0) == pb.n - 4 * pb.m
        v, dn = pb.newton()
        assert np.array_equal(pb.A @ dn + pb.b, np.zeros(pb.m))
        g = pb.A.T @ pb.b
        Ag = pb.A @ g
        for what, terms in (("newton", dn * dn), ("gg", g * g), ("AgAg", Ag * Ag)):
            _assert_integer_sum(terms, what)
        assert -np.sum(g * g) / np.sum(Ag * Ag) == -0.125
        assert np.any(dn != -0.125 * g)           # (the Cauchy point is not the Newton point)
        c_v = (pb.A @ pb.c) / pb.aat_diag()
        ref = cc.stage_refresh(pb.A, pb.c, pb.b, c_v)
        assert np.array_equal(ref["ct"] * 64, np.round(ref["ct"] * 64))
        assert np.array_equal(pb.A @ ref["ct"], np.zeros(pb.m))


def test_judge_rungs_are_reached(capsys):
    for m in cc.JUDGE_M:
        b_next = cc.judge_b_next(m)
        _assert_integer_sum(b_next ** 2, ("judge", m))
        assert np.sum(b_next ** 2) > 0
        for rung in cc.JUDGE_RUNGS:
            q, f_next = cc.judge_case(rung, b_next)
            out = cc.stage_judge(q, b_next, f_next)
            assert cc.judge_rung_reached(out, q) == rung, (m, rung, out)
            if rung.startswith("shrink"):
                assert out[cc.ACCEPT] == 0.0 and out[cc.PENALTY] == q[cc.PREV_PENALTY] != q[cc.PENALTY]
            if rung == "soc":
                assert (out[cc.ACCEPT], out[cc.RADIUS], out[cc.PENALTY]) == (0.0, q[cc.RADIUS],
                                                                             q[cc.PENALTY])
    with capsys.disabled():
        for rung in cc.JUDGE_RUNGS:
            print("judge rung %-16s <- judge_case(%r), m in %s" % (rung, rung, cc.JUDGE_M))


@pytest.mark.parametrize("name", DISJOINT)
def test_newton_and_dogleg_branches_are_reached(name, capsys):
    pb = problem(name)
    _, dn = pb.newton()
    lines = []
    for case, kind in cc.NEWTON_CASES.items():
        radius, lb, ub = cc.newton_case(pb, case)
        out = cc.stage_newton(dn, lb, ub, radius)
        assert out[cc.NORMAL_KIND] == kind, (case, out)
        if case == "ball":
            assert out[cc.NVIOL] == 0 and out[cc.NORM_DN] > cc.TR_FACTOR * radius
        if case in ("box-lb", "box-ub"):
            assert out[cc.NVIOL] == 1 and out[cc.NORM_DN] <= cc.TR_FACTOR * radius
        if case == "equal-ball":
            assert out[cc.NORM_DN] == cc.TR_FACTOR * radius
        if case == "equal-box":
            assert np.sum(dn == cc.BOX_FACTOR * lb) == 1 and np.sum(dn == cc.BOX_FACTOR * ub) == 1
        lines.append("newton check %-12s kind %d <- newton_case(%s, %r)" % (case, kind, name, case))
    assert np.isnan(cc.stage_given(pb.dn, 0.5)[cc.RADIUS_T])          # ||dn|| > radius
    for case in cc.DOGLEG_CASES:
        radius, lb, ub = cc.dogleg_case(pb, case)
        nw = cc.stage_newton(dn, lb, ub, radius)
        if case == "stands":
            assert nw[cc.NORMAL_KIND] == 1.0
            lines.append("dogleg %-14s <- dogleg_case(%s, %r)" % ("newton-stands", name, case))
            continue
        assert nw[cc.NORMAL_KIND] == 0.0, case
        out = cc.stage_dogleg(pb, pb.b, lb, ub, radius)
        assert out["branch"] == cc.DOGLEG_CASES[case], (case, out["branch"], out["block"])
        assert out["block"][cc.DOGLEG] == -0.125
        scale = np.maximum(np.abs(out["oracle_dn"]), np.abs(out["dn"]))
        assert np.all(np.abs(out["dn"] - out["oracle_dn"]) <= 4 * np.spacing(scale))
        if out["branch"][1] == "x2":
            assert out["r2"] < out["r1"] * (1 - 1e-3)
        if out["branch"][1] == "x1":
            assert out["r1"] < out["r2"] * (1 - 1e-3)
        if case == "tie":
            assert out["r1"] == out["r2"] and out["block"][cc.DOGLEG + 4] == 2.0
        lines.append("dogleg %-13s won by %-3s <- dogleg_case(%s, %r)" % (out["branch"] + (name, case)))
    with capsys.disabled():
        print("\n".join(lines))


@pytest.mark.parametrize("name", SMALL + ["slots"])
def test_exit_branches_are_reached(name, capsys):
    pb = problem(name)
    lines = []
    for case in cc.EXIT_CASES:
        stop, alpha, radius, z, p, lbt, ubt = cc.exit_case(pb, case)
        out = cc.stage_exit(stop, alpha, radius, z, p, lbt, ubt)
        kind = case.rsplit("-", 1)[0]
        if kind == "plain":
            assert out["done"] == 0.0 and out["tau"] == 0.0
            assert cc.inside_count(z, lbt, ubt) == 1
        else:
            lo, hi = lbt, ubt
            d = (alpha if stop == 2 else 1.0) * p
            with np.errstate(all="ignore"):
                _, _, _, sph, box = cc.oqp.box_sphere_intersections(z, d, lo, hi, radius, stop == 3,
                                                                    extra_info=True)
            if kind == "box":
                assert out["hit"] and out["tau"] > 0 and box["tb"] < sph["tb"] * (1 - cc.MARGIN)
            if kind == "sphere":
                assert out["hit"] and out["tau"] > 0 and sph["tb"] < box["tb"] * (1 - cc.MARGIN)
            if kind == "miss":
                assert not out["hit"] and out["tau"] == 0.0 and out["done"] == 1.0
                assert np.sum((p == 0) & ((z < lbt) | (z > ubt))) == 2
                assert not np.array_equal(cc.clip_step(z, 0.0, p, lbt, ubt), z)
        lines.append("exit %-9s stop %d tau %-22r <- exit_case(%s, %r)" % (kind, stop, out["tau"],
                                                                          name, case))
    with capsys.disabled():
        print("\n".join(lines))


@pytest.mark.parametrize("name", SMALL)
def test_model_cases_show_what_they_name(name):
    pb = problem(name)
    assert pb.on_bound > 0                                      # entries exactly on a bound
    assert cc.inside_count(pb.dt, pb.lbt, pb.ubt) == len(pb.outside) > 1
    assert cc.inside_count(pb.dt, pb.lbt, None) == len(pb.outside) // 2
    assert cc.inside_count(pb.dt, None, pb.ubt) == len(pb.outside) - len(pb.outside) // 2
    nan = pb.dt.copy()
    nan[7] = np.nan
    assert cc.inside_count(nan, pb.lbt, pb.ubt) == cc.inside_count(pb.dt, pb.lbt, pb.ubt) + \
        (0 if 7 in pb.outside else 1)


@pytest.mark.parametrize("name", ["one", "two"])
def test_tolerance_tier_decisions_keep_their_margin(name, capsys):
    inst = cc.tolerance_instance(name)
    _, dn = cc.tolerance_newton(inst)
    for case in ("accepted", "ball", "box"):
        radius, lb, ub, kind = cc.tolerance_newton_case(inst, case)
        assert min(cc.newton_margins(dn, radius, lb, ub)) >= cc.MARGIN, case
        assert cc.stage_newton(dn, lb, ub, radius)[cc.NORMAL_KIND] == kind
        with capsys.disabled():
            print("tolerance newton check %-9s kind %d <- tolerance_newton_case(%s, %r)"
                  % (case, kind, name, case))
