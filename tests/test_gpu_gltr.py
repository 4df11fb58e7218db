"""csrc/gltr.hip on the device: the tridiagonal trust-region solve against its host twin, and
ipx_gltr_start / _step / _combine against the numpy expressions they stand for (exactly on
small-integer data, within n 2^-53 sum|terms| for the reductions on real data, bit for bit for
the elementwise parts), with the stop word honoured by later steps."""
import ctypes
import math
import types

import numpy as np
import pytest

import gltr_cases
from test_gltr_host import tridiag_host

pytestmark = pytest.mark.gpu

HDR = 16
U = 2.0 ** -53


@pytest.fixture(scope="module")
def gpu():
    import torch
    from ipsolver import _hip, device as dv
    return types.SimpleNamespace(hip=_hip, dv=dv, lib=_hip.load(), torch=torch)


def dev(gpu, a):
    return gpu.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def test_tridiagonal_solve_matches_its_host_twin(gpu):
    """Equal case flags and exit paths, lambda and h within 1e-12 relative (the host runs the
    device's lanes one after the other: the same operations; bitwise agreement is counted)."""
    cases = gltr_cases.tridiagonals()
    outs = []
    for diag, off, g0, R in cases:
        k = len(diag)
        out = gpu.torch.zeros(8 + k, dtype=gpu.torch.float64, device="cuda")
        d, o = dev(gpu, diag), dev(gpu, off if k > 1 else np.zeros(1))
        gpu.hip.call("ipx_gltr_tridiag", k, d.data_ptr(), o.data_ptr(), g0, R, out.data_ptr(),
                     gpu.dv.stream_ptr())
        outs.append(out)
    bitwise = 0
    for idx, ((diag, off, g0, R), out) in enumerate(zip(cases, outs)):
        got = out.cpu().numpy()
        ref = tridiag_host(diag, off, g0, R)
        assert int(got[3]) == ref["case"] and int(got[4]) == ref["path"], (idx, got[:6], ref)
        assert abs(got[0] - ref["lam"]) <= 1e-12 * abs(ref["lam"]), (idx, got[0], ref["lam"])
        h = got[8:]
        assert np.linalg.norm(h - ref["h"]) <= 1e-12 * np.linalg.norm(ref["h"]), idx
        bitwise += int(np.array_equal(h, ref["h"]) and got[0] == ref["lam"])
    print("bitwise equal to the host twin: %d of %d" % (bitwise, len(cases)))


def _alloc(gpu, n, kmax):
    t = gpu.torch
    lib = gpu.lib
    Q = t.full((n * (kmax + 1) + 2,), float("nan"), dtype=t.float64, device="cuda")
    state = t.full((int(lib.ipx_gltr_state_doubles(kmax)),), float("nan"), dtype=t.float64,
                   device="cuda")
    part = t.zeros(int(lib.ipx_gltr_part_doubles(n)), dtype=t.float64, device="cuda")
    return Q, state, part


def _start(gpu, n, kmax, cap, g, Q, state, part, R, tol):
    gd = dev(gpu, g)
    gpu.hip.call("ipx_gltr_start", n, kmax, cap, gd.data_ptr(), Q.data_ptr(), state.data_ptr(),
                 part.data_ptr(), R, tol, gpu.dv.stream_ptr())


def _step(gpu, n, kmax, w, Q, state, part):
    wd = dev(gpu, w)
    gpu.hip.call("ipx_gltr_step", n, kmax, wd.data_ptr(), Q.data_ptr(), state.data_ptr(),
                 part.data_ptr(), gpu.dv.stream_ptr())
    gpu.torch.cuda.synchronize()


def _combine(gpu, n, kmax, Q, state, x0, offset=0):
    t = gpu.torch
    buf = t.full((n + 4,), float("nan"), dtype=t.float64, device="cuda")
    x = buf[2 + offset:2 + offset + n]
    x0d = None
    if x0 is not None:
        x0buf = t.full((n + 4,), float("nan"), dtype=t.float64, device="cuda")
        x0d = x0buf[2 + offset:2 + offset + n]
        x0d.copy_(dev(gpu, x0))
    gpu.hip.call("ipx_gltr_combine", n, kmax, Q.data_ptr(), state.data_ptr(),
                 None if x0d is None else x0d.data_ptr(), x.data_ptr(), gpu.dv.stream_ptr())
    got = buf.cpu().numpy()
    assert np.isnan(got[:2 + offset]).all() and np.isnan(got[2 + offset + n:]).all()
    return got[2 + offset:2 + offset + n]


def _combine_ref(Q, n, h, x0):
    x = np.zeros(n) if x0 is None else x0.copy()
    for j in range(len(h)):
        x = x + h[j] * Q[j * n:(j + 1) * n]
    return x


SIZES = (1, 63, 257, 4099, 4100, 70001)


@pytest.mark.parametrize("kmax", [1, 2, 64])
@pytest.mark.parametrize("n", SIZES)
def test_start_step_combine_on_real_data(gpu, n, kmax):
    rng = np.random.default_rng(100 * n + kmax)
    g = rng.standard_normal(n)
    R, tol = 0.7, 0.0
    Q, state, part = _alloc(gpu, n, kmax)
    _start(gpu, n, kmax, kmax, g, Q, state, part, R, tol)
    st = state.cpu().numpy()
    gg = math.fsum(g * g)
    assert abs(st[2] ** 2 - gg) <= (n + 4) * U * gg
    assert st[0] == 0 and st[1] == 0 and st[3] == R and st[4] == tol and st[10] == kmax
    assert not st[HDR:].any()
    Qh = Q.cpu().numpy()
    assert np.array_equal(Qh[:n], g / st[2])
    assert np.isnan(Qh[n * (kmax + 1):]).all()
    steps = min(kmax, 4 if n > 1 else 1)
    for k in range(steps):
        w = rng.standard_normal(n)
        _step(gpu, n, kmax, w, Q, state, part)
        st = state.cpu().numpy()
        Qh = Q.cpu().numpy()
        diag, off = st[HDR:HDR + kmax], st[HDR + kmax:HDR + 2 * kmax]
        assert st[1] == k + 1
        qk = Qh[k * n:(k + 1) * n]
        terms = qk * w
        assert abs(diag[k] - math.fsum(terms)) <= n * U * np.abs(terms).sum()
        v = w - diag[k] * qk
        if k > 0:
            v = v - off[k - 1] * Qh[(k - 1) * n:k * n]
        vv = math.fsum(v * v)
        assert abs(off[k] ** 2 - vv) <= (n + 4) * U * vv
        assert st[8] == off[k]
        col = Qh[(k + 1) * n:(k + 2) * n]
        if st[0] == 0:
            assert np.array_equal(col, v / off[k])
        else:
            assert np.array_equal(col, v)              # (the step that stops does not normalise)
        assert np.isnan(Qh[n * (kmax + 1):]).all()
        # the tridiagonal problem of this step, as the host twin solves it
        if off[k] > 1e-14 * st[2] or k > 0:
            ref = tridiag_host(diag[:k + 1], off[:k], st[2], R)
            h = st[HDR + 2 * kmax:HDR + 2 * kmax + k + 1]
            assert int(st[9]) == ref["case"] and int(st[11]) == ref["path"]
            assert np.linalg.norm(h - ref["h"]) <= 1e-12 * np.linalg.norm(ref["h"])
            assert abs(st[5] - ref["lam"]) <= 1e-12 * abs(ref["lam"])
            assert abs(st[7] - ref["q"]) <= 1e-12 * abs(ref["q"])
        if st[0] != 0:
            break
    st = state.cpu().numpy()
    if steps == kmax or n == 1:
        assert st[0] in (1.0, 4.0)
        if n == 1:
            assert st[0] == 4.0 and st[8] == 0.0          # w - (q'w) q = 0: invariant subspace
        elif st[0] == 1.0:
            assert st[1] == kmax
    # a step after the stop, or simply one more: state and Q are checked for the former
    if st[0] != 0:
        before_s, before_q = state.clone(), Q.clone()
        for _ in range(2):
            _step(gpu, n, kmax, rng.standard_normal(n), Q, state, part)
        assert gpu.torch.equal(before_s.view(gpu.torch.int64), state.view(gpu.torch.int64))
        assert gpu.torch.equal(before_q.view(gpu.torch.int64), Q.view(gpu.torch.int64))
    # x = x0 + Q h, bit for bit, with and without x0, at both alignments of x and x0
    k = int(st[1])
    h = st[HDR + 2 * kmax:HDR + 2 * kmax + k]
    Qh = Q.cpu().numpy()
    x0 = rng.standard_normal(n)
    for offset in (0, 1):
        assert np.array_equal(_combine(gpu, n, kmax, Q, state, None, offset),
                              _combine_ref(Qh, n, h, None))
        assert np.array_equal(_combine(gpu, n, kmax, Q, state, x0, offset),
                              _combine_ref(Qh, n, h, x0))


@pytest.mark.parametrize("n", SIZES)
def test_first_step_is_exact_on_small_integers(gpu, n):
    """gamma_0, q_0, delta_0, the new column and gamma_1^2 are exact when every term is a small
    dyadic number: g with 4^j entries +-1 (gamma_0 = 2^j), w of small integers."""
    rng = np.random.default_rng(n)
    kmax = 2
    j = 0
    while 4 ** (j + 1) <= min(n, 256):
        j += 1
    g = np.zeros(n)
    idx = rng.permutation(n)[:4 ** j]
    g[idx] = rng.choice([-1.0, 1.0], 4 ** j)
    w = rng.integers(-8, 9, n).astype(float)
    Q, state, part = _alloc(gpu, n, kmax)
    _start(gpu, n, kmax, kmax, g, Q, state, part, 1.0, 0.0)
    _step(gpu, n, kmax, w, Q, state, part)
    st = state.cpu().numpy()
    Qh = Q.cpu().numpy()
    q0 = g / 2.0 ** j
    assert st[2] == 2.0 ** j and np.array_equal(Qh[:n], q0)
    delta = float(np.sum(q0 * w))
    v = w - delta * q0
    assert st[HDR] == delta
    assert st[HDR + kmax] == math.sqrt(float(np.sum(v * v)))
    col = Qh[n:2 * n]
    if st[0] == 0:
        assert np.array_equal(col, v / st[HDR + kmax])
    else:
        assert np.array_equal(col, v)


def test_early_stop_and_argument_checks(gpu):
    n, kmax = 257, 4
    rng = np.random.default_rng(1)
    g = rng.standard_normal(n)
    Q, state, part = _alloc(gpu, n, kmax)
    # gamma_0^2 below the tolerance: stop code 4, no vector, and steps change nothing
    _start(gpu, n, kmax, kmax, g, Q, state, part, 1.0, 1e9)
    st = state.cpu().numpy()
    assert st[0] == 4 and st[1] == 0
    before_s, before_q = state.clone(), Q.clone()
    _step(gpu, n, kmax, g, Q, state, part)
    assert gpu.torch.equal(before_s.view(gpu.torch.int64), state.view(gpu.torch.int64))
    assert gpu.torch.equal(before_q.view(gpu.torch.int64), Q.view(gpu.torch.int64))
    assert np.array_equal(_combine(gpu, n, kmax, Q, state, g), g)
    # the default tolerance is projected_cg's
    _start(gpu, n, kmax, kmax, g, Q, state, part, 1.0, -1.0)
    st = state.cpu().numpy()
    assert st[4] == max(min(0.01 * st[2], 0.1 * (st[2] * st[2])), 1e-25) or \
        abs(st[4] - max(min(0.01 * st[2], 0.1 * st[2] ** 2), 1e-25)) <= 4 * U * st[4]
    # a cap below kmax stops with code 1 at the cap
    _start(gpu, n, kmax, 2, g, Q, state, part, 1e-3, 0.0)
    for _ in range(3):
        _step(gpu, n, kmax, rng.standard_normal(n), Q, state, part)
    st = state.cpu().numpy()
    assert st[0] == 1 and st[1] == 2
    lib = gpu.lib
    P = ctypes.c_void_p
    assert lib.ipx_gltr_step(n, 257, P(Q.data_ptr()), P(Q.data_ptr()), P(state.data_ptr()),
                             P(part.data_ptr()), None) < 0
    assert lib.ipx_gltr_step(0, kmax, P(Q.data_ptr()), P(Q.data_ptr()), P(state.data_ptr()),
                             P(part.data_ptr()), None) < 0
