"""Constructed operands and plain numpy transcriptions of the stages of csrc/sqp.hip
(``ipx_sqp_front`` / ``_model`` / ``_judge`` / ``_refresh``), for tests/test_gpu_sqp_chain_stages.py
(device) and tests/test_sqp_chain_cases_host.py (what the cases claim, without a device).
numpy and scipy only.

Two tiers of data.

Exact tier.  Every vector holds small integers times powers of two (|value| <= 8), H is
tridiagonal and symmetric with integer entries, and A has DISJOINT rows: row i holds four entries
in columns 4i..4i+3, +-1 on even rows and +-2 on odd rows, so A A' = diag(4, 16, 4, 16, ...).  With
a diagonal A A' of powers of two the solve (A A')^-1 b, the Newton point -A'(A A')^-1 b and
g = A'b are exact, and every sum a kernel forms is an integer multiple of a fixed power of two
far below 2^53: the same bits in any order of addition, so the expected block entries are known
without reference to the kernels' grids.  b is chosen with sum b^2 over even rows = 8 x the sum
over odd rows, which makes the Cauchy coefficient -(g.g)/(Ag.Ag) exactly -1/8.

Tolerance tier.  Random real data (tests/banded_setup.BandedInstance) for what a diagonal A A'
cannot show; references are taken in extended precision from the device's own input vectors and
the bound is ``sum_tolerance`` below.

The block's ownership list (which SQ_* entries each entry point writes; csrc/sqp.hip's comment
block on the SQ_* enum refers here) is ``OWNED``.
"""
import math

import numpy as np
import scipy.sparse as sps

import oracle.qp_subproblem as oqp

# ---- the block (csrc/sqp.hip SQ_*; test_sqp_chain_cases_host.py checks these against sqp_chain) --
(RADIUS, PENALTY, F, NORM_B, NORM_DN, RADIUS_T, NORMAL_KIND, NVIOL, HDD, CD, LIN, NORM_D, NORM_DT,
 QMODEL, VPRED, PREV_PENALTY, PRED, MERIT, F_NEXT, NORM_B_NEXT, ACTUAL, RATIO, SOC, ACCEPT, OPT,
 VIOL, NORM_A2, FACTOR_BAD, EXIT_TAU, EXIT_DONE, X_OUTSIDE, PRIME_STEPS) = range(32)
CG, DOGLEG, SIZE = 32, 48, 64
ST_RADIUS, ST_ALPHA, ST_STOP = 3, 4, 5          # csrc/cg.hip ST_* (ipsolver/cg_fused.py)
TR_FACTOR, BOX_FACTOR = 0.8, 0.5

_MODEL = [HDD, CD, LIN, NORM_D, NORM_DT, QMODEL, VPRED, PREV_PENALTY, PRED, MERIT, PENALTY, F,
          NORM_B, X_OUTSIDE, PRIME_STEPS] + list(range(CG, CG + 16))
_NORMAL = [NVIOL, NORM_DN, NORMAL_KIND, RADIUS, RADIUS_T]
# entries of the block each entry point (and form) writes; every other entry keeps its bits
OWNED = {
    "judge": [F_NEXT, NORM_B_NEXT, ACTUAL, RATIO, SOC, ACCEPT, RADIUS, PENALTY],
    "model_host_cg": _MODEL,
    "model": _MODEL + [EXIT_TAU, EXIT_DONE],
    "front": _MODEL + [EXIT_TAU, EXIT_DONE] + _NORMAL,
    "front_dogleg": _MODEL + [EXIT_TAU, EXIT_DONE] + _NORMAL + list(range(DOGLEG, DOGLEG + 7)),
    "refresh": [OPT, VIOL, NORM_B, FACTOR_BAD],
    "refresh_norm_A": [OPT, VIOL, NORM_B, FACTOR_BAD, NORM_A2],
}


def sentinels():
    """64 distinct doubles no stage computes."""
    return -(4096.0 + np.arange(SIZE)) - 0.28125


# ---- grids -----------------------------------------------------------------------------------
def grid_for(n):
    """csrc/ipx_common.h ipx_grid_for(n, 4 * 256): workgroups of the chains' vector kernels."""
    return min(max((n + 1023) // 1024, 1), 1024)


def depth(n):
    """The longest chain of additions a term passes through in a chain reduction over n elements:
    grid-stride trips, 8 levels of the block reduction, 12 of the fold."""
    return -(-n // (grid_for(n) * 256)) + 8 + 12


def sum_tolerance(terms, n=None, d=None):
    """2 D 2^-53 sum |terms|."""
    terms = np.asarray(terms, dtype=np.float64)
    d = depth(len(terms) if n is None else n) if d is None else d
    return 2.0 * d * 2.0 ** -53 * math.fsum(np.abs(terms))


# name -> (n, m, kind of exact A, (g, gm))
SHAPES = {
    "one": (600, 60, "disjoint", (1, 1)),
    "two": (1025, 104, "disjoint", (2, 1)),
    "few": (5000, 1250, "disjoint", (5, 2)),
    # g = 258 and gm = 257 leave no room for rows of four (n >= 4m): rows 4 e_i + e_{i+1}
    "slots": (263200, 262200, "chain", (258, 257)),
    # ... and the same n with disjoint rows for the stages whose exactness needs them
    "slots_n": (263200, 65800, "disjoint", (258, 65)),
    "capped": (1048576 + 1025, 262400, "disjoint", (1024, 257)),
}


def _ints(rng, n, hi=8):
    return rng.integers(-hi, hi + 1, n).astype(np.float64)


def exact_A(n, m, kind):
    i = np.arange(m)
    if kind == "disjoint":
        assert n >= 4 * m and n - m >= 1
        sign = np.array([[1, -1, 1, 1], [-1, -1, 1, -1], [1, 1, -1, 1]], dtype=np.float64)
        val = sign[i % 3] * np.where(i % 2 == 0, 1.0, 2.0)[:, None]
        col = 4 * i[:, None] + np.arange(4)[None, :]
        ptr = 4 * np.arange(m + 1)
    else:
        assert n >= m + 1
        val = np.tile(np.array([4.0, 1.0]), (m, 1))
        col = i[:, None] + np.arange(2)[None, :]
        ptr = 2 * np.arange(m + 1)
    return sps.csr_matrix((val.ravel(), col.ravel().astype(np.int32), ptr.astype(np.int32)),
                          shape=(m, n))


def exact_H(n):
    i = np.arange(n)
    diag = 2.0 + (i % 3)
    off = np.where(i[:-1] % 2 == 0, 1.0, -2.0)
    H = sps.diags([off, diag, off], [-1, 0, 1], format="csr")
    H.indices = H.indices.astype(np.int32)
    H.indptr = H.indptr.astype(np.int32)
    return H


def cauchy_b(m, rng):
    """Integers with sum b_i^2 over even rows = 8 x the sum over odd rows (needs m >= 6): odd rows
    +-1; even rows (4, 0) by pairs, one triple (2, 2, 4) when their count is odd, an extra even row
    (odd m) 0."""
    assert m >= 6
    b = np.zeros(m)
    n_odd = m // 2
    b[1::2] = rng.choice([-1.0, 1.0], n_odd)
    ev = np.zeros(n_odd)                       # (an odd m's last even row stays 0)
    k = n_odd
    if k % 2:
        ev[k - 3:] = [2.0, 2.0, 4.0]
        k -= 3
    ev[0:k:2] = 4.0
    ev *= rng.choice([-1.0, 1.0], n_odd)
    b[0:2 * n_odd:2] = ev
    assert np.sum(b[0::2] ** 2) == 8 * np.sum(b[1::2] ** 2)
    return b


class ExactProblem:
    """Operands of the exact tier for one shape (host arrays; the device test uploads them)."""

    def __init__(self, name):
        n, m, kind, grids = SHAPES[name]
        self.name, self.n, self.m, self.kind, self.grids = name, n, m, kind, grids
        rng = np.random.default_rng(1000 + len(name) + n)
        self.A, self.H = exact_A(n, m, kind), exact_H(n)
        self.x, self.c = _ints(rng, n) * 0.5, _ints(rng, n)
        self.b = cauchy_b(m, rng) if kind == "disjoint" else _ints(rng, m)
        self.scale = rng.choice([0.5, 1.0, 2.0], n)
        self.dn = _ints(rng, n, 4) * 0.5
        self.dt = _ints(rng, n, 4)
        self.p = _ints(rng, n, 8)
        self.b_next = _ints(rng, m, 8) * 0.25
        # shifted bounds around dt: 0 .. 4 away (0: exactly on the bound, inside), a few outside
        self.lbt = self.dt - rng.integers(0, 5, n)
        self.ubt = self.dt + rng.integers(0, 5, n)
        self.outside = np.unique(rng.integers(0, n, 5))
        half = len(self.outside) // 2
        self.lbt[self.outside[:half]] += 7.0
        self.ubt[self.outside[half:]] -= 7.0
        self.on_bound = int(np.sum((self.lbt == self.dt) | (self.ubt == self.dt)))
        # trust bounds of the step (front): wide, so that a case narrows single entries
        self.lb, self.ub = np.full(n, -64.0), np.full(n, 64.0)

    # the normal step's exact pieces (disjoint rows)
    def aat_diag(self):
        assert self.kind == "disjoint"
        return np.where(np.arange(self.m) % 2 == 0, 4.0, 16.0)

    def newton(self, b=None):
        b = self.b if b is None else b
        v = b / self.aat_diag()
        return v, -(self.A.T @ v)


class RowSpace:
    """Y of the oracle's modified_dogleg for a disjoint-row A: A'(A A')^-1."""

    def __init__(self, pb):
        self.pb = pb

    def dot(self, b):
        return self.pb.A.T @ (b / self.pb.aat_diag())


# ---- the reference statements of the decisions (tests/test_sqp_decisions.py), reused ------------
def _decisions():
    import test_sqp_decisions as t
    return t._model_ref, t._ladder_ref


# ---- stage transcriptions ---------------------------------------------------------------------
def inside_count(t, lo, hi):
    """Box violations as the kernels count them: a NaN is outside."""
    lo = -np.inf if lo is None else lo
    hi = np.inf if hi is None else hi
    with np.errstate(invalid="ignore"):
        return float(np.sum(~((lo <= t) & (t <= hi))))


def stage_refresh(A, c, b, v):
    """``v`` = (A A')^-1 A c as the device's solve left it (or the exact value).  c + A'(-v) with
    each row's products summed, then subtracted from c; the norms of b."""
    ct = c - (A.T @ v)
    return {"v_out": -v, "ct": ct,
            "block": {OPT: float(np.max(np.abs(ct))), VIOL: float(np.max(np.abs(b))),
                      NORM_B: float(np.sqrt(np.sum(b * b)))}}


def stage_newton(dn, lb, ub, radius):
    """k_sq_newton_check + sq_after_newton on a Newton point ``dn`` (qp_subproblem.py:368-373)."""
    lo = None if lb is None else BOX_FACTOR * lb
    hi = None if ub is None else BOX_FACTOR * ub
    nviol = inside_count(dn, lo, hi) if (lb is not None or ub is not None) else 0.0
    norm_dn = float(np.sqrt(np.sum(dn * dn)))
    ok = nviol == 0.0 and norm_dn <= TR_FACTOR * radius
    with np.errstate(invalid="ignore"):
        rt = float(np.sqrt(np.float64(radius * radius - norm_dn * norm_dn)))
    return {NVIOL: nviol, NORM_DN: norm_dn, NORMAL_KIND: 1.0 if ok else 0.0, RADIUS: radius,
            RADIUS_T: rt}


def stage_given(dn, radius):
    norm_dn = float(np.sqrt(np.sum(dn * dn)))
    with np.errstate(invalid="ignore"):
        rt = float(np.sqrt(np.float64(radius * radius - norm_dn * norm_dn)))
    return {NVIOL: 0.0, NORM_DN: norm_dn, NORMAL_KIND: 2.0, RADIUS: radius, RADIUS_T: rt}


def stage_dogleg(pb, b, lb, ub, radius):
    """qp_subproblem.py:375-413 on a disjoint-row problem, the intersections by the oracle:
    reduce (coefficient), decide (mode, alphas), points, take (winner)."""
    n = pb.n
    lo = np.full(n, -np.inf) if lb is None else BOX_FACTOR * lb
    hi = np.full(n, np.inf) if ub is None else BOX_FACTOR * ub
    tr = TR_FACTOR * radius
    A = pb.A
    _, newton = pb.newton(b)
    g = A.T @ b
    Ag = A @ g
    coef = -np.dot(g, g) / np.dot(Ag, Ag)
    cauchy = coef * g
    origin = np.zeros(n)
    with np.errstate(all="ignore"):
        _, a1, hit1 = oqp.box_sphere_intersections(cauchy, newton - cauchy, lo, hi, tr)
        _, a2, _ = oqp.box_sphere_intersections(origin, cauchy, lo, hi, tr)
        _, a3, _ = oqp.box_sphere_intersections(origin, newton, lo, hi, tr)
    x1 = cauchy + a1 * (newton - cauchy) if hit1 else origin + a2 * cauchy
    x2 = origin + a3 * newton
    r1, r2 = np.linalg.norm(A @ x1 + b), np.linalg.norm(A @ x2 + b)
    first = bool(r1 < r2)
    dn = x1 if first else x2
    with np.errstate(all="ignore"):
        ref = oqp.modified_dogleg(A, RowSpace(pb), b, tr, lo, hi)
    branch = ("segment" if hit1 else "scaled-cauchy",
              "x1" if first else ("tie" if r1 == r2 else "x2"))
    return {"dn": dn, "oracle_dn": ref, "branch": branch, "r1": r1, "r2": r2,
            "block": {DOGLEG: coef, DOGLEG + 1: 1.0 if hit1 else 0.0,
                      DOGLEG + 2: float(a1 if hit1 else a2), DOGLEG + 3: float(a3),
                      DOGLEG + 4: 1.0 if first else 2.0, DOGLEG + 5: float(r1),
                      DOGLEG + 6: float(r2)}}


def stage_ct_bounds(H, c, dn, lb, ub):
    """c_t = H dn + c and the shifted bounds."""
    return {"ct": H @ dn + c, "lbt": None if lb is None else lb - dn,
            "ubt": None if ub is None else ub - dn}


def stage_exit(stop, alpha, radius, z, p, lbt, ubt):
    """k_sq_exit_reduce: the boundary exits of the CG loop (:565-568, :588-590) by the oracle's
    box_sphere_intersections."""
    if stop not in (2, 3):
        return {"done": 0.0, "tau": 0.0, "hit": None}
    n = len(z)
    lo = np.full(n, -np.inf) if lbt is None else lbt
    hi = np.full(n, np.inf) if ubt is None else ubt
    d = (alpha if stop == 2 else 1.0) * p
    with np.errstate(all="ignore"):
        _, tb, hit = oqp.box_sphere_intersections(z, d, lo, hi, radius, entire_line=stop == 3)
    tau = 0.0 if not hit else float(tb * alpha if stop == 2 else tb)
    return {"done": 1.0, "tau": tau, "hit": bool(hit)}


def clip_step(dt, tau, p, lbt, ubt):
    """k_sq_step_vectors' move along p and clip (tau == 0: dt itself, clipped)."""
    t = dt + tau * p if tau != 0.0 else dt.copy()
    if lbt is not None:
        t = np.maximum(t, lbt)
    if ubt is not None:
        t = np.minimum(t, ubt)
    return t


def stage_model(pb, dn, dt, lbt, ubt, scale, penalty, f, norm_b, prime_steps=0.0):
    """k_sq_step_vectors (without the exit), H d, A d + b, k_sq_model_sums, :135-153."""
    d = dn + dt
    x_next = pb.x + (scale * d if scale is not None else d)
    Hd, Ad = pb.H @ d, pb.A @ d + pb.b
    terms = {NORM_D: d * d, NORM_DT: dt * dt, CD: pb.c * d, HDD: Hd * d, LIN: Ad * Ad}
    blk = {NORM_D: float(np.sqrt(np.sum(d * d))), NORM_DT: float(np.sqrt(np.sum(dt * dt))),
           CD: float(np.sum(pb.c * d)), HDD: float(np.sum(Hd * d)),
           LIN: float(np.sqrt(np.sum(Ad * Ad))),
           X_OUTSIDE: inside_count(dt, lbt, ubt) if (lbt is not None or ubt is not None) else 0.0,
           PRIME_STEPS: prime_steps, F: f, NORM_B: norm_b}
    blk.update(model_entries(blk[HDD], blk[CD], blk[LIN], norm_b, penalty, f))
    return {"d": d, "x_next": x_next, "Hd": Hd, "Ad": Ad, "block": blk, "terms": terms}


def model_entries(hdd, cd, lin, norm_b, penalty, f):
    model_ref, _ = _decisions()
    qm, vpred, prev, pen, pred, merit = model_ref(hdd, cd, lin, norm_b, penalty, f)
    return {QMODEL: qm, VPRED: vpred, PREV_PENALTY: prev, PENALTY: pen, PRED: pred, MERIT: merit}


def stage_judge(q, b_next, f_next):
    """k_sq_judge_norms on a block ``q`` (indexable by SQ_*): :156-173, the ladder :196-242."""
    _, ladder_ref = _decisions()
    with np.errstate(invalid="ignore"):
        nbn = float(np.sqrt(np.sum(b_next * b_next))) if len(b_next) else 0.0
    actual = q[MERIT] - (f_next + q[PENALTY] * nbn)
    ratio = actual / q[PRED]
    soc = bool(ratio < 1e-8 and q[NORM_DN] <= 0.1 * q[NORM_DT])
    out = {F_NEXT: f_next, NORM_B_NEXT: nbn, ACTUAL: actual, RATIO: ratio, SOC: 1.0 if soc else 0.0}
    if soc:
        out.update({ACCEPT: 0.0, RADIUS: q[RADIUS], PENALTY: q[PENALTY]})
    else:
        r, acc, pen = ladder_ref(ratio, q[NORM_D], q[RADIUS], q[PENALTY], q[PREV_PENALTY])
        out.update({ACCEPT: 1.0 if acc else 0.0, RADIUS: r, PENALTY: pen})
    return out


# ---- cases ------------------------------------------------------------------------------------
# judge: name -> (target ratio, norm_d, radius, norm_dn, norm_dt); penalty 1, prev penalty 0.5,
# pred 1, merit 100
JUDGE_RUNGS = {
    "large": (0.95, 1.0, 2.0, 1.0, 1.0),
    "intermediary": (0.5, 2.0, 2.0, 1.0, 1.0),
    "sufficient": (0.1, 1.0, 2.0, 1.0, 1.0),
    "shrink-half": (-1.0, 4.0, 2.0, 1.0, 1.0),
    "shrink-to-step": (-1.0, 1.0, 2.0, 1.0, 1.0),
    "shrink-tenth": (-1.0, 0.125, 2.0, 1.0, 1.0),
    "soc": (-1.0, 1.0, 2.0, 1.0, 16.0),
}
JUDGE_M = [1, 2, 3] + sorted({s[1] for s in SHAPES.values()})


def judge_b_next(m):
    rng = np.random.default_rng(77 + m)
    return _ints(rng, m, 8) * 0.25 + (0.25 if m < 4 else 0.0)


def judge_case(rung, b_next):
    """(block inputs, f_next): f_next puts actual / predicted at the rung's target."""
    ratio, norm_d, radius, norm_dn, norm_dt = JUDGE_RUNGS[rung]
    q = {MERIT: 100.0, PENALTY: 1.0, PREV_PENALTY: 0.5, PRED: 1.0, NORM_D: norm_d, RADIUS: radius,
         NORM_DN: norm_dn, NORM_DT: norm_dt}
    nbn = float(np.sqrt(np.sum(b_next * b_next)))
    return q, 100.0 - nbn - ratio


def judge_rung_reached(out, q):
    """Which rung of :196-212 a judged block took."""
    if out[SOC]:
        return "soc"
    r = out[RATIO]
    if r >= 0.9:
        return "large"
    if r >= 0.3:
        return "intermediary"
    if r >= 1e-8:
        return "sufficient"
    if out[RADIUS] == 0.5 * q[RADIUS]:
        return "shrink-half"
    if out[RADIUS] == 0.1 * q[RADIUS]:
        return "shrink-tenth"
    return "shrink-to-step"


def exit_case(pb, name):
    """Operands of ipx_sqp_model with host_cg = 0: (stop, alpha, radius, z, p, lbt, ubt).
    box-*: the box limits the step; sphere-*: the ball does; miss-*: zero entries of p, some of
    them outside the box."""
    kind, stop = name.rsplit("-", 1)
    stop = int(stop)
    n = pb.n
    rng = np.random.default_rng(5 + n)
    z = _ints(rng, n, 2) * 0.5
    p = _ints(rng, n, 8)
    p[rng.random(n) < 0.1] = 0.0
    p[0] = 8.0
    lbt, ubt = z - 3.0, z + 5.0
    alpha = 0.5 if stop == 2 else 0.0
    zz = float(np.sum(z * z))
    if kind == "box":
        radius = 1048576.0
    elif kind == "sphere":
        radius = float(np.sqrt(zz)) + 0.25
    elif kind == "miss":
        radius = 1048576.0
        j = np.flatnonzero(p == 0.0)[:3]
        assert len(j) == 3
        lbt = lbt.copy()
        lbt[j[0]] = z[j[0]] + 1.0
        ubt = ubt.copy()
        ubt[j[1]] = z[j[1]] - 2.0
    else:
        assert kind == "plain"              # stop codes 0, 1, 4: no exit, nothing moved or clipped
        radius = 1048576.0
        lbt = lbt.copy()
        lbt[1] = z[1] + 1.0                 # (an entry outside the box stays where it is)
    return stop, alpha, radius, z, p, lbt, ubt


EXIT_CASES = ["plain-0", "plain-1", "plain-4", "box-2", "sphere-2", "miss-2", "box-3", "sphere-3",
              "miss-3"]


def equal_radius(norm_dn):
    """A radius with fl(0.8 radius) == norm_dn exactly (the ball test's equality)."""
    r = norm_dn / TR_FACTOR
    for _ in range(8):
        t = TR_FACTOR * r
        if t == norm_dn:
            return r
        r = np.nextafter(r, np.inf if t < norm_dn else -np.inf)
    raise AssertionError("no radius with 0.8 r == %r" % norm_dn)


def newton_case(pb, name):
    """(radius, lb, ub) of a Newton-check case on the exact problem."""
    _, dn = pb.newton()
    norm_dn = float(np.sqrt(np.sum(dn * dn)))
    lb, ub = pb.lb.copy(), pb.ub.copy()
    neg, pos = int(np.flatnonzero(dn < 0)[-1]), int(np.flatnonzero(dn > 0)[-1])
    radius = 4.0 * norm_dn
    if name == "ball":
        radius = norm_dn
    elif name == "box-lb":
        lb[neg] = dn[neg]                   # 0.5 lb > dn there
    elif name == "box-ub":
        ub[pos] = dn[pos]
    elif name == "equal-ball":
        radius = equal_radius(norm_dn)
    elif name == "equal-box":
        lb[neg], ub[pos] = 2.0 * dn[neg], 2.0 * dn[pos]
    else:
        assert name == "accepted"
    return radius, lb, ub


NEWTON_CASES = {"accepted": 1.0, "ball": 0.0, "box-lb": 0.0, "box-ub": 0.0, "equal-ball": 1.0,
                "equal-box": 1.0}


def dogleg_case(pb, name):
    """(radius, lb, ub) of a dogleg case.  With O = the sum of b^2 over the odd rows this data has
    ||cauchy||^2 = 3/4 O and ||newton||^2 = 33/16 O; on the columns of an even row cauchy = newton
    / 2, on those of an odd row cauchy = 2 newton; ||A x + b||^2 is 3 O (1 - a)^2 at cauchy +
    a (newton - cauchy), O (9 - 12 a + 6 a^2) at a cauchy and 9 O (1 - a)^2 at a newton -- under
    the ball alone the scaled Newton point always wins, the box decides the other way."""
    O = float(np.sum(pb.b[1::2] ** 2))
    _, dn = pb.newton()
    lb, ub = pb.lb.copy(), pb.ub.copy()
    radius = 64.0 * np.sqrt(O)
    even_pos = int(np.flatnonzero(dn == 1.0)[0])          # a column of an even row with b = -+4
    odd_pos = int(np.flatnonzero(dn == 0.125)[0])         # ... of an odd row
    if name == "stands":
        pass
    elif name == "segment":
        # newton = 1/8 below the box (0.5 lb = 3/16), cauchy = 1/4 inside: the segment leaves the
        # box at alpha = 1/2, the line from the origin never reaches it below t = 1 (x2 = 0)
        lb[odd_pos] = 0.375
    elif name == "scaled-cauchy":
        # 0.5 ub = 1/4 against cauchy = 1/2, newton = 1: alpha 1/2 along cauchy, 1/4 along newton
        ub[even_pos] = 0.5
    elif name == "x2":
        # 0.5 ub = 3/4: the segment is cut at alpha = 1/2, the line from the origin at 3/4
        ub[even_pos] = 1.5
    elif name == "ball":
        radius = np.sqrt(O) / TR_FACTOR             # cauchy inside, newton outside the ball
    elif name == "ball-cauchy":
        radius = np.sqrt(0.5 * O) / TR_FACTOR       # the Cauchy point outside as well
    elif name == "tie":
        # a bound of 0 against the direction of both candidates: both end at the origin
        ub[even_pos] = 0.0
    else:
        raise AssertionError(name)
    return float(radius), lb, ub


# case -> (how x1 is formed, who wins)
DOGLEG_CASES = {"stands": None, "segment": ("segment", "x1"), "scaled-cauchy": ("scaled-cauchy", "x1"),
                "x2": ("segment", "x2"), "ball": ("segment", "x2"),
                "ball-cauchy": ("scaled-cauchy", "x2"), "tie": ("scaled-cauchy", "tie")}


# ---- tolerance tier -----------------------------------------------------------------------------
TOL_SHAPES = {"one": (600, 60), "two": (1025, 104), "few": (5000, 1250)}
MARGIN = 1e-6


def tolerance_instance(name):
    from banded_setup import BandedInstance
    return BandedInstance(*TOL_SHAPES[name])


def tolerance_newton(inst):
    """The Newton point of the instance in float64 on the host (to place the thresholds)."""
    A = inst.A.tocsr()
    S = (A @ A.T).tocsc()
    import scipy.sparse.linalg as spla
    v = spla.spsolve(S, inst.b)
    return v, -(A.T @ v)


def tolerance_newton_case(inst, name):
    """(radius, lb, ub, expected NORMAL_KIND): thresholds placed from the host's Newton point with
    wide margins."""
    _, dn = tolerance_newton(inst)
    norm_dn, amax = float(np.linalg.norm(dn)), float(np.max(np.abs(dn)))
    n = inst.n
    lb, ub = np.full(n, -8.0 * amax), np.full(n, 8.0 * amax)
    if name == "accepted":
        return 4.0 * norm_dn, lb, ub, 1.0
    if name == "ball":
        return 0.5 * norm_dn, lb, ub, 0.0
    assert name == "box"
    j = int(np.argmax(np.abs(dn)))
    if dn[j] > 0:
        ub[j] = dn[j]
    else:
        lb[j] = dn[j]
    return 4.0 * norm_dn, lb, ub, 0.0


def newton_margins(dn, radius, lb, ub):
    """Relative distances of the Newton check's comparisons from their thresholds."""
    norm_dn = float(np.linalg.norm(dn))
    tr = TR_FACTOR * radius
    out = [abs(norm_dn - tr) / tr]
    for bound in (lb, ub):
        t = BOX_FACTOR * bound
        out.append(float(np.min(np.abs(dn - t) / np.maximum(np.abs(t), np.abs(dn)))))
    return out
