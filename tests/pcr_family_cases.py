"""What the cyclic-reduction kernels of csrc/banded.hip (k_pcr_check, k_solve_pcr,
k_step1_solve_tail) compute, case by case, as arrays to be compared BIT FOR BIT with
tests/golden/pcr_family_bits.npz (tests/test_gpu_pcr_family_bits.py; written by
``tests/golden/make_golden.py --pcr-family`` on the GPU).

Every case is a function without arguments that returns ``{key: numpy array}``.  A vector of more
than DIGEST_OVER entries is stored as a digest: its words as unsigned 64-bit integers, summed
(wrapping) over consecutive groups of 64 -- a change of any bit of any entry changes its group's
sum, and the fixture of all cases stays far below 1 MiB.
"""
import ctypes
import os

import numpy as np
import scipy.sparse as sps

DIGEST_OVER = 512
LOOP_FIELDS = ("x", "r", "p", "Hp", "v", "state")
SIZES = [1820, 2080, 2340, 4421, 6500]          # 7, 8, 9, 18, 25 windows of 260 rows


def digest(a):
    a = np.ascontiguousarray(a)
    if a.size <= DIGEST_OVER:
        return a.copy()
    words = a.view(np.uint64).ravel()
    pad = (-words.size) % 64
    words = np.concatenate((words, np.zeros(pad, np.uint64)))
    return words.reshape(-1, 64).sum(axis=1, dtype=np.uint64)


class forms:
    """IPX_DEBUG_FORMS for the duration of a block."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.saved = os.environ.get("IPX_DEBUG_FORMS")
        if self.value is None:
            os.environ.pop("IPX_DEBUG_FORMS", None)
        else:
            os.environ["IPX_DEBUG_FORMS"] = self.value

    def __exit__(self, *exc):
        if self.saved is None:
            os.environ.pop("IPX_DEBUG_FORMS", None)
        else:
            os.environ["IPX_DEBUG_FORMS"] = self.saved


# ------------------------------------------------------------------ the projection of the CG loop
def two_iterations(q, fused, form, radius=1e300):
    """A bare loop object on problem ``q`` (test_gpu_projection_placement.Problem), primed on the
    host, two iterations: the loop's vectors, its state block and the partials of the projection."""
    import torch
    import ipsolver.cg_fused as cg_fused
    import ipsolver.device as dv
    from ipsolver import _hip
    import test_gpu_projection_placement as pp
    with forms(form):
        L = cg_fused._Loop(q.H, q.P, None, None, resident=False, fused_projection=fused)
        # (without the ELL(2) form of A' -- an odd n -- the tail runs in k_solve_decoupled)
        assert not L.args.resident and L.args.At_qv > 0 and L.args.At_ell_val
        assert L.args.fused_proj == (1 if fused else 0)
        nwin = L.geometry[2]
        pp.prime(L, q, radius=radius)
        _hip.check(_hip.load().ipx_cg_iterate(L.ref(), 0, 2, dv.stream_ptr()), "ipx_cg_iterate")
        torch.cuda.synchronize()
        assert int(L.state[cg_fused.ST_STOP].item()) == 0
        assert int(L.state[cg_fused.ST_IT_DONE].item()) == 2
    out = {name: digest(getattr(L, name).cpu().numpy()) for name in LOOP_FIELDS}
    out["part3"] = L.part3[:2 * nwin].cpu().numpy().copy()
    out["part4"] = L.part4[:nwin].cpu().numpy().copy()
    out["tail_lanes"] = np.array([int(L.args.At_qv), nwin])
    return out


def _tagged(tag, d):
    return {tag + "." + k: v for k, v in d.items()}


def projection_forms(m):
    """k_step1_solve_tail<6, 0 / 2, false, true> (the first iteration reads x and p, the second
    one folds the carried sums), the same with the 16-bit column table, and the separate launches
    with k_solve_pcr<6, 1>: the bits of each."""
    import test_gpu_projection_placement as pp
    q = pp.problem(m)
    out = {}
    out.update(_tagged("fused", two_iterations(q, True, "no-resident")))
    out.update(_tagged("table", two_iterations(q, True, "no-resident,table-columns")))
    out.update(_tagged("three", two_iterations(q, False, "no-resident")))
    return out


def projection_radius_forms():
    """XN = 0 in both iterations (``read-xn2``) and XN = 1 (no radius), fused and separate."""
    import test_gpu_projection_placement as pp
    q = pp.problem(2340)
    out = {}
    for tag, fused in (("fused", True), ("three", False)):
        out.update(_tagged(tag + ".xn0", two_iterations(q, fused, "no-resident,read-xn2")))
        out.update(_tagged(tag + ".xn1", two_iterations(q, fused, "no-resident",
                                                        radius=float("inf"))))
    return out


def priming_projection():
    """qp.projected_cg at m = 2340, three iterations, second call on the same Jacobian (the one
    that arms the fused projection before the priming: k_step1_solve_tail<.., PRIME> with sign
    +1, then -1), and the same with ``no-fused-projection``."""
    import ipsolver.cg_fused as cg_fused
    import ipsolver.qp as qp
    import test_gpu_projection_placement as pp
    q = pp.problem(2340)
    saved = cg_fused.resident_limits
    limits = dict(saved(), max_wg=4)
    cg_fused.resident_limits = lambda: limits
    out = {}
    try:
        for tag, form in (("fused", "no-resident"), ("three", "no-resident,no-fused-projection")):
            with forms(form):
                for call in range(2):
                    x, info = qp.projected_cg(q.H, q.c, q.Z, q.Y, np.zeros(q.m),
                                              trust_radius=1e300, tol=0, max_iter=3)
                L = next(reversed(cg_fused._POOL.values()))
                assert int(L.args.fused_proj) == (1 if tag == "fused" else 0)
                out[tag + ".x"] = digest(x.t.cpu().numpy())
                out[tag + ".info"] = np.array([info["niter"], info["stop_cond"],
                                               int(info["hits_boundary"])])
    finally:
        cg_fused.resident_limits = saved
    return out


# ------------------------------------------------------- k_solve_pcr's tail at every compiled width
def strided_rows(m, bw, stride2):
    """Row i: ``bw`` entries of size about 1 from column floor(i stride2 / 2) on; bw <= stride2:
    A A' is tridiagonal and a variable sees at most two constraints, in adjacent rows.  Rows
    share at most a quarter of their columns: couplings of at most ~0.3 of the diagonal, which
    the reduction has below 2^-56 by level 6."""
    rng = np.random.default_rng(bw * 1000 + stride2)
    start = (np.arange(m) * stride2) // 2
    n = int(start[-1]) + bw
    cols = (start[:, None] + np.arange(bw)[None, :]).ravel()
    A = sps.csr_matrix((rng.uniform(0.9, 1.1, m * bw) * rng.choice([-1.0, 1.0], m * bw),
                        (np.repeat(np.arange(m), bw), cols)), shape=(m, n))
    A.sort_indices()
    off = rng.uniform(-0.4, 0.4, n - 1)
    H = sps.diags([off, rng.uniform(1.5, 2.5, n), off], [-1, 0, 1], format="csr")
    return A, H, rng.standard_normal(n)


# (row length, twice the column stride, rows): 780, 1560 and 2990 variables per window of 260
# rows -- 2, 4 and 7 per lane of the tail's 512, the instantiations QV = 2, 4 and 8 (QV = 6: the
# problems of ``projection_forms``).  The row counts make n even, which the pair tail needs.
TAIL_WIDTHS = {2: (4, 6, 1301), 4: (8, 12, 1300), 8: (14, 23, 1300)}


def solve_tail_width(qv):
    import test_gpu_projection_placement as pp
    from ipsolver import _hip
    bw, stride2, m = TAIL_WIDTHS[qv]
    A, H, c = strided_rows(m, bw, stride2)
    assert A.shape[1] % 2 == 0
    q = pp.Problem(A.tocsr(), H.tocsr(), c)
    out = two_iterations(q, False, "no-resident")
    level = int(_hip.load().ipx_banded_pcr_level(ctypes.c_void_p(q.P.solver.handle)))
    out["level"] = np.array([level])
    per_lane = (int(out["tail_lanes"][0]) * 192 + 1 + 511) // 512
    assert level > 0 and qv - 2 < per_lane <= qv, (qv, level, out["tail_lanes"])
    return out


# --------------------------------------------------- the plain solve and the factor-time level search
def toeplitz_band(m, diag, sub):
    band = np.empty(2 * m)
    band[:m] = diag
    band[m:] = sub
    band[m] = 0.0
    return band


def moving_average_band(m, W, eps):
    """The band of S = A A' for test_gpu_normal_solve.moving_average(m, 1, W, eps)."""
    return toeplitz_band(m, 2.0 * W * W + eps * eps, 1.0 * W * W)


# one matrix per outcome of k_pcr_check; the first three are the matrices of
# test_gpu_normal_solve.test_cyclic_reduction_decision_edges and its ramp's unscaled blocks
LEVEL_CASES = {
    "low": lambda m: toeplitz_band(m, 2.0 + 49.0, 1.0),          # rows 1, 1, private 7
    "L6": lambda m: moving_average_band(m, 8, 7),
    "L7": lambda m: moving_average_band(m, 36, 22),
    "separators_coupled": lambda m: moving_average_band(m, 36, 12),   # (distance 65; 128 is not)
    "coupled": lambda m: moving_average_band(m, 36, 6),          # still coupled at distance 128
    "indefinite": lambda m: toeplitz_band(m, 1.0, 0.75),         # |2 sub| > diag: not SPD
}


def reduction_model(band, levels=7):
    """numpy model of k_pcr_check on one window in the interior of a Toeplitz S (IEEE divisions
    for the kernel's reciprocal): per level s = 0 .. levels - 1 the largest coupling at distance
    2^(s+1) over 2^-56 of the reduced diagonal."""
    m = len(band) // 2
    size = 1024
    b = np.full(size, band[m // 2])
    a = np.full(size, band[m + m // 2])
    a[0] = 0.0
    out = []
    mid = slice(size // 2 - 8, size // 2 + 8)
    for s in range(levels):
        h = 1 << s
        r = 1.0 / b
        lo = lambda v, fill: np.concatenate((np.full(h, fill), v[:-h]))      # noqa: E731
        hi = lambda v, fill: np.concatenate((v[h:], np.full(h, fill)))       # noqa: E731
        al, ga = -a * lo(r, 1.0), -hi(a, 0.0) * hi(r, 1.0)
        b = b + al * a + ga * hi(a, 0.0)
        a = al * lo(a, 0.0)
        out.append(float(np.max(np.abs(a[mid]) / (2.0 ** -56 * b[mid]))))
    return out


def level_search(name):
    """ipx_banded_create / factor / status on a band handed over directly: the status, the
    level and the decoupling verdict; where the reduction is the solve, x of ipx_banded_solve
    (k_solve_pcr without partials) and x, partials of ipx_banded_solve_resid."""
    import torch
    import ipsolver.device as dv
    from ipsolver import _hip
    m = 3000
    lib, st = _hip.load(), dv.stream_ptr()
    band = torch.from_numpy(LEVEL_CASES[name](m)).cuda()
    h = ctypes.c_void_p(lib.ipx_banded_create(m, 1, 64))
    assert h.value
    out = {}
    try:
        _hip.call("ipx_banded_factor", h, dv._p(band), st)
        status = int(lib.ipx_banded_status(h, st))
        level = int(lib.ipx_banded_pcr_level(h))
        geo = (ctypes.c_int32 * 2)()
        dec = int(lib.ipx_banded_decoupled_geometry(h, geo))
        out["verdict"] = np.array([status, level, int(lib.ipx_banded_decoupled(h)), dec,
                                   geo[0] if dec else 0, geo[1] if dec else 0])
        if level > 0:
            w = torch.from_numpy(np.random.default_rng(5).standard_normal(m)).cuda()
            x = torch.full((m,), float("nan"), dtype=torch.float64, device="cuda")
            _hip.call("ipx_banded_solve", h, dv._p(w), dv._p(x), st)
            out["solve.x"] = digest(x.cpu().numpy())
            x = torch.full((m,), float("nan"), dtype=torch.float64, device="cuda")
            part = torch.full((geo[1] + 8,), -7.25, dtype=torch.float64, device="cuda")
            npart = ctypes.c_int32(0)
            _hip.call("ipx_banded_solve_resid", h, dv._p(w), dv._p(x), dv._p(part),
                      ctypes.byref(npart), None, st)
            assert npart.value == geo[1]
            out["resid.x"] = digest(x.cpu().numpy())
            out["resid.partials"] = part.cpu().numpy()
    finally:
        lib.ipx_banded_destroy(h)
    return out


# ------------------------------------------------------------------------------- the tail forms
def two_sided_box():
    """The general rows of test_gpu_projection_placement.box_schur_nine_windows (2340 rows of 15
    entries, 8 columns apart) with a lower AND an upper bound row on every variable: the group
    tables are then computed, not read, which the per-item tail of the Schur solve needs."""
    rng = np.random.default_rng(2341)
    rl, shift, m = 15, 8, 2340
    n = (m - 1) * shift + rl
    cols = (np.arange(m)[:, None] * shift + np.arange(rl)[None, :]).ravel()
    J = sps.csr_matrix((rng.uniform(0.5, 1.5, m * rl) * rng.choice([-1.0, 1.0], m * rl),
                        (np.repeat(np.arange(m), rl), cols)), shape=(m, n))
    I = sps.eye(n, format="csr")
    s = rng.uniform(1e-6, 2.0, m + 2 * n)
    A = sps.bmat([[J, sps.diags(s[:m]), None, None], [-I, None, sps.diags(s[m:m + n]), None],
                  [I, None, None, sps.diags(s[m + n:])]], format="csr")
    A.sort_indices()
    M, N = A.shape
    off = rng.uniform(-0.4, 0.4, n - 1)
    Hx = sps.diags([off, rng.uniform(1.5, 2.5, n), off], [-1, 0, 1], format="csr")
    Hz = sps.block_diag([Hx, sps.diags(rng.uniform(0.5, 2.0, N - n))], format="csr")
    lb = np.concatenate((np.full(n, -np.inf), np.full(N - n, -0.995)))
    return A, Hz, rng.standard_normal(N), np.zeros(M), lb, \
        dict(trust_radius=np.inf, tol=1e-10, max_iter=40)


def box_schur(post):
    """k_solve_pcr forming its own right-hand side (ROWS): on the nine-window box-Schur problem of
    test_gpu_projection_placement (bounds on one side: no per-item tail), and with the per-item
    tail (ROWS + POST) on ``two_sided_box``; four iterations of the public loop."""
    import ipsolver.device as dv
    import ipsolver.projector as projector
    import ipsolver.cg_fused as cg_fused
    import test_gpu_projection_placement as pp
    A, Hz, c, b, lb, kw = two_sided_box() if post else pp.box_schur_nine_windows()
    with forms(None):
        Z, _, Y = projector.projections(dv.DeviceCSR.from_scipy(A))
        solver = Z.projector.solver
        assert type(solver).__name__ == "BoxSchurNormalSolver"
        args = solver.c_args()
        assert args.AR_rowlen == 16 and bool(args.post_own_g) == post
        x, info = cg_fused.projected_cg(dv.DeviceCSR.from_scipy(Hz), dv.DVec.from_host(c), Z, Y,
                                        dv.DVec.from_host(b), lb=dv.DVec.from_host(lb),
                                        **dict(kw, max_iter=4))
    return {"x": digest(x.to_host()),
            "info": np.array([info["niter"], info["stop_cond"], int(info["hits_boundary"])])}


CASES = {}
for _m in SIZES:
    CASES["projection_m%d" % _m] = (lambda m=_m: projection_forms(m))
CASES["projection_radius"] = projection_radius_forms
CASES["priming"] = priming_projection
for _qv in sorted(TAIL_WIDTHS):
    CASES["tail_qv%d" % _qv] = (lambda qv=_qv: solve_tail_width(qv))
for _name in LEVEL_CASES:
    CASES["level_" + _name] = (lambda name=_name: level_search(name))
CASES["rows_post"] = lambda: box_schur(True)
CASES["rows"] = lambda: box_schur(False)


def record(log=print, only=None):
    """Every case -> {"<case>/<key>": array}; a case whose expectations do not hold is reported
    and left out (an error of the device library ends the recording)."""
    out, failed = {}, []
    for name, fn in CASES.items():
        if only and name not in only:
            continue
        try:
            got = fn()
        except AssertionError as e:
            failed.append(name)
            log("case %s: NOT RECORDED: assertion %r" % (name, e))
            continue
        for k, v in got.items():
            out[name + "/" + k] = v
        log("case %s: %d arrays, %d bytes" % (name, len(got), sum(v.nbytes for v in got.values())))
    return out, failed
