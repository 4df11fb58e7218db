"""Limited-memory quasi-Newton approximations of the objective's Hessian: ``hess=LBFGS()`` or
``hess=LSR1()`` in ``minimize_constrained``, for problems that have no Hessian callback.

The objects hold parameters only.  Every solve starts from an empty memory (``_Memory``), so two
solves with the same object give the same bits.  They are deliberately not callable: the
solver's ``callable(hess)`` branches never take them for a Hessian callback.

Both rules keep the compact form ``B = sigma I + W C W'`` with ``W = [S Y]`` on the device
(csrc/lowrank.hip): S and Y are two rings of ``memory`` columns in one buffer, sigma and the
signs are folded into C, and a product is ``B p = sigma p + W (C (W'p))`` -- two HBM-bound
passes over W, no host involvement.  An update is three launches and reads nothing back.

Only the objective is approximated: constraint Hessians still come from their callbacks, from
finite differences or are absent, exactly as without a strategy.
"""
import numbers

import numpy as np

MAX_MEMORY = 32            # IPX_LR_MAX_MEMORY: r = 2 memory <= 64 columns
KIND_LBFGS, KIND_LSR1 = 0, 1


def _check(memory, init_scale, threshold, what):
    if isinstance(memory, bool) or not isinstance(memory, numbers.Integral) \
            or not 1 <= memory <= MAX_MEMORY:
        raise ValueError("memory must be an integer between 1 and %d, got %r"
                         % (MAX_MEMORY, memory))
    if not (isinstance(init_scale, str) and init_scale == 'auto'):
        if isinstance(init_scale, (bool, str)) or not isinstance(init_scale, numbers.Real) \
                or not np.isfinite(init_scale) or init_scale <= 0:
            raise ValueError("init_scale must be 'auto' or a positive finite number, got %r"
                             % (init_scale,))
    if isinstance(threshold, (bool, str)) or not isinstance(threshold, numbers.Real) \
            or not np.isfinite(threshold) or threshold < 0:
        raise ValueError("%s must be a non-negative finite number, got %r" % (what, threshold))


class _Strategy:
    kind = None

    @property
    def init_value(self):
        """sigma the kernels take: > 0 given, 0 = 'auto'"""
        return 0.0 if isinstance(self.init_scale, str) else float(self.init_scale)

    def __repr__(self):
        return "%s(memory=%d, init_scale=%r, %s=%r)" % (
            type(self).__name__, self.memory, self.init_scale, self._threshold_name,
            self.threshold)


class LBFGS(_Strategy):
    """Limited-memory BFGS approximation of the objective's Hessian.

    Compact form of Byrd, Nocedal & Schnabel (1994) over the stored pairs (oldest first)::

        B = sigma I - [sigma S  Y] [[sigma S'S, L], [L', -D]]^-1 [sigma S'; Y']

    with ``L`` the strictly lower triangle of ``S'Y`` and ``D`` its diagonal.

    Update rule.  Each time the solver asks for the Lagrangian Hessian at a new accepted ``x``,
    ``s = x - x_prev`` and ``y = grad f(x) - grad f(x_prev)``, ``x_prev`` the point of the last
    update and both gradients the ones the solver already evaluated (no extra gradient calls).
    ``s = 0`` (the same point again, as across barrier levels) is not an update and is not
    counted.  The pair is stored when ``s'y > min_curvature ||s|| ||y||``, otherwise skipped
    and counted in ``hess_skipped``; when the memory is full the oldest pair is dropped.
    ``sigma = y'y / s'y`` of the newest stored pair for ``init_scale='auto'`` (1 before the
    first), else ``init_scale``.  The middle matrix is inverted by Gauss-Jordan with partial
    pivoting; a pivot at or below ``1e-14 max|entry|`` skips the pair too (a guard: with every
    ``s'y > 0`` the matrix is invertible).

    Limitation: only the objective is approximated, and a pair is only stored along steps of
    positive curvature.  On an objective with negative curvature along the steps the solver
    takes (the Coulomb energy of ``Elec`` in the test problems) every pair after the first few is
    skipped, ``B`` stops changing and the solve can run out of iterations; ``LSR1`` stores
    such pairs.

    Parameters
    ----------
    memory : int, 1 <= memory <= 32
        Pairs kept.
    init_scale : 'auto' or float > 0
    min_curvature : float >= 0
    """
    kind = KIND_LBFGS
    _threshold_name = "min_curvature"

    def __init__(self, memory=10, init_scale='auto', min_curvature=1e-8):
        _check(memory, init_scale, min_curvature, "min_curvature")
        self.memory = int(memory)
        self.init_scale = init_scale
        self.min_curvature = float(min_curvature)

    @property
    def threshold(self):
        return self.min_curvature


class LSR1(_Strategy):
    """Limited-memory symmetric rank-one approximation of the objective's Hessian.

    Compact form over the stored pairs (oldest first)::

        B = sigma I + (Y - sigma S) (D + L + L' - sigma S'S)^-1 (Y - sigma S)'

    with ``L`` the strictly lower triangle of ``S'Y`` and ``D`` its diagonal.

    Update rule.  ``s``, ``y``, ``x_prev`` and the ``s = 0`` case as for ``LBFGS``.  ``sigma``
    is fixed at the first stored pair -- ``y'y / s'y`` when that is positive, else 1 -- or is
    ``init_scale``; before a pair is stored, each candidate is tested against ``sigma I`` with
    the sigma it would fix.  The pair is stored when ``|s'(y - Bs)| >= min_denominator ||s||
    ||y - Bs||`` (and ``s'(y - Bs) != 0``), ``B`` the current approximation, and the new middle
    matrix inverts by Gauss-Jordan with partial pivoting with every pivot above
    ``1e-14 max|entry|``; otherwise it is skipped and counted.  When the memory is full the
    oldest pair is dropped.  ``s'Bs`` and ``||y - Bs||`` follow from the Gram of ``[S Y]`` and
    ``C`` (no extra pass over the vectors).

    Parameters
    ----------
    memory : int, 1 <= memory <= 32
    init_scale : 'auto' or float > 0
    min_denominator : float >= 0
    """
    kind = KIND_LSR1
    _threshold_name = "min_denominator"

    def __init__(self, memory=10, init_scale='auto', min_denominator=1e-8):
        _check(memory, init_scale, min_denominator, "min_denominator")
        self.memory = int(memory)
        self.init_scale = init_scale
        self.min_denominator = float(min_denominator)

    @property
    def threshold(self):
        return self.min_denominator


def is_strategy(hess):
    return isinstance(hess, _Strategy)


class LowRankTerm:
    """The objective's term ``B`` of the Lagrangian Hessian: an x-space device operator
    (``backend_hip.hessian_operator`` pads it in z-space).  A view of the memory: valid until
    the memory's next update, which is the next Hessian the solver asks for."""
    device_operator = True
    lowrank_term = True

    def __init__(self, memory):
        self.mem = memory
        self.shape = (memory.n, memory.n)

    def dot(self, p, out=None, accumulate=False):
        from . import _hip
        from .device import DVec, _empty, _p, stream_ptr
        m = self.mem
        if out is None:
            out = DVec(_empty(m.n))
            accumulate = False
        _hip.call("ipx_lowrank_apply", m.n, m.strategy.memory, _p(m.W), _p(m.state), _p(p.t),
                  _p(out.t), 1 if accumulate else 0, _p(m.part), stream_ptr())
        return out

    matvec = dot


class _Memory:
    """One solve's memory of a strategy on the device: W (n x 2 memory), the state block, the
    partial-sum scratch; the last update's point and gradient."""

    def __init__(self, strategy, n):
        import torch
        from . import _hip
        from .device import ctx
        lib = _hip.load()
        self.strategy, self.n = strategy, int(n)
        dev = ctx().device
        M = strategy.memory
        self.W = torch.zeros(2 * M * self.n, dtype=torch.float64, device=dev)
        st = np.zeros(lib.ipx_lowrank_state_doubles(M))
        st[0] = strategy.init_value if strategy.init_value > 0 else 1.0
        self.state = torch.from_numpy(st).to(dev)
        self.part = torch.empty(lib.ipx_lowrank_part_doubles(self.n, M), dtype=torch.float64,
                                device=dev)
        self.x_prev = self.g_prev = None
        self.term = LowRankTerm(self)

    def observe(self, x, g):
        """The solver asks for the Hessian at ``x`` (DVec) whose gradient is ``g`` (DVec):
        update with (x - x_prev, g - g_prev) unless it is the first point."""
        from . import _hip
        from .device import stream_ptr, _p
        if self.x_prev is not None:
            s, y = x - self.x_prev, g - self.g_prev
            st = self.strategy
            _hip.call("ipx_lowrank_update", st.kind, self.n, st.memory, st.init_value,
                      st.threshold, _p(self.W), _p(s.t), _p(y.t), _p(self.state), _p(self.part),
                      stream_ptr())
        # copies: the caller's vectors may be buffers it writes again
        self.x_prev, self.g_prev = x.copy(), g.copy()
        return self.term

    def counts(self):
        """(updates, skipped) -- one blocking read, at the end of a solve"""
        from .device import read_doubles
        v = read_doubles(self.state, 2, offset=3)
        return int(v[0]), int(v[1])


def host_hessian(strategy, grad, n):
    """``hess`` for host-callback mode: x (numpy) -> the objective's term.  ``grad`` is the
    memoised gradient (minimize._Memoize), so the gradient at an accepted point is the one the
    solver evaluated there."""
    from .device import DVec
    memory = _Memory(strategy, n)
    last = {"x": None}

    def hess(x):
        if last["x"] is not None and np.array_equal(x, last["x"]):
            return memory.term                  # the same point again: not an update
        last["x"] = np.array(x, dtype=float, copy=True)
        return memory.observe(DVec.from_host(x), DVec.from_host(grad(x)))
    return hess, memory


class DeviceGradientMemo:
    """Device-callback mode: the user's gradient callback with copies of its last few points and
    its results kept.  The solver evaluates the gradient at every accepted point before it asks for
    the Hessian there, so a lookup finds it; the point is compared by value (one blocking read
    per Hessian: the solver reuses device buffers, which a tensor's storage address or version
    does not see).  A lookup that misses calls the callback."""

    KEEP = 4

    def __init__(self, grad):
        self.grad = grad
        self._seen = []                 # (point, gradient), newest first
        self.misses = 0                 # lookups that had to call the callback

    def __call__(self, xt):
        g = self.grad(xt)
        # copies of both: the solver reuses its buffers, a callback may reuse its output
        import torch
        gt = g if torch.is_tensor(g) else g.t
        self._seen = [(xt.detach().clone(), gt.detach().clone())] + self._seen[:self.KEEP - 1]
        return g

    def lookup(self, xt):
        import torch
        for x, g in self._seen:
            if xt.shape == x.shape and bool(torch.equal(xt, x)):
                return g
        self.misses += 1
        return self(xt)


def device_hessian(strategy, memo, n):
    """``hess`` for device-callback mode: CUDA tensor -> the objective's term.  The same point
    again gives s = 0, which the update kernel ignores."""
    from . import device_mode as dm
    memory = _Memory(strategy, n)

    def hess(xt):
        g = memo.lookup(xt)
        return memory.observe(dm.as_dvec(xt), dm.as_dvec(g))
    return hess, memory
