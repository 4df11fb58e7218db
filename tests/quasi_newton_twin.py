"""numpy twin of ipsolver.LBFGS / ipsolver.LSR1: the compact forms and update rules of their
docstrings over explicit vectors, the dense recursions they stand for, and a host model of the
device memory (W, the state block) driven by ``ipx_lowrank_middle_host``."""
import ctypes

import numpy as np

HDR = 16          # IPX_LR_HDR


class CompactTwin:
    """kind 0: L-BFGS, 1: L-SR1; init_scale None = 'auto'."""

    def __init__(self, kind, memory, init_scale=None, threshold=1e-8):
        self.kind, self.memory, self.init, self.thr = kind, memory, init_scale, threshold
        self.S, self.Y = [], []
        self.sigma = init_scale if init_scale is not None else 1.0
        self.sigma_fixed = False
        self.updates = self.skipped = 0

    def _middle(self, S, Y, sigma):
        S, Y = np.array(S).T, np.array(Y).T
        SY = S.T @ Y
        L, D = np.tril(SY, -1), np.diag(np.diag(SY))
        if self.kind == 0:
            return np.block([[sigma * S.T @ S, L], [L.T, -D]])
        return D + L + L.T - sigma * S.T @ S

    def _invertible(self, Mid):
        # Gauss-Jordan with partial pivoting, every pivot above 1e-14 max|entry|
        a = Mid.copy()
        amax = np.max(np.abs(a))
        K = a.shape[0]
        for p in range(K):
            r = p + int(np.argmax(np.abs(a[p:, p])))
            if not abs(a[r, p]) > 1e-14 * amax:
                return False
            a[[p, r]] = a[[r, p]]
            a[p] /= a[p, p]
            for i in range(K):
                if i != p:
                    a[i] -= a[i, p] * a[p]
        return True

    def B(self, n=None):
        n = n if n is not None else (len(self.S[0]) if self.S else None)
        if not self.S:
            return self.sigma * np.eye(n)
        return self._compact(self.S, self.Y, self.sigma, n)

    def _compact(self, Sl, Yl, sigma, n):
        return self._apply(Sl, Yl, sigma, np.eye(n))

    def _apply(self, Sl, Yl, sigma, P):
        """B P for the pairs (Sl, Yl) without forming B"""
        if not Sl:
            return sigma * P
        S, Y = np.array(Sl).T, np.array(Yl).T
        Mid = self._middle(Sl, Yl, sigma)
        if self.kind == 0:
            Wm = np.hstack((sigma * S, Y))
            return sigma * P - Wm @ np.linalg.solve(Mid, Wm.T @ P)
        V = Y - sigma * S
        return sigma * P + V @ np.linalg.solve(Mid, V.T @ P)

    def dot(self, p):
        return self._apply(self.S, self.Y, self.sigma, np.asarray(p, float))

    def update(self, s, y):
        s, y = np.asarray(s, float), np.asarray(y, float)
        n = len(s)
        ss, sy, yy = s @ s, s @ y, y @ y
        if ss == 0:
            return
        if self.kind == 0:
            ok = sy > self.thr * np.sqrt(ss * yy)
            sigma = self.init if self.init is not None else yy / sy
        else:
            if self.sigma_fixed:
                sigma = self.sigma
            elif self.init is not None:
                sigma = self.init
            else:
                sigma = yy / sy if sy > 0 and yy / sy > 0 else 1.0
            r = y - self._apply(self.S, self.Y, sigma, s)
            den = s @ r
            ok = abs(den) > 0 and abs(den) >= self.thr * np.sqrt(ss * (r @ r))
        S, Y = (self.S + [s])[-self.memory:], (self.Y + [y])[-self.memory:]
        if ok:
            ok = self._invertible(self._middle(S, Y, sigma))
        if not ok:
            self.skipped += 1
            return
        self.S, self.Y, self.sigma = S, Y, sigma
        self.sigma_fixed = True
        self.updates += 1


def dense_recursion(kind, S, Y, sigma):
    """B from sigma I by the BFGS / SR1 update over the pairs, oldest first."""
    n = len(S[0])
    B = sigma * np.eye(n)
    for s, y in zip(S, Y):
        Bs = B @ s
        if kind == 0:
            B = B - np.outer(Bs, Bs) / (s @ Bs) + np.outer(y, y) / (s @ y)
        else:
            r = y - Bs
            B = B + np.outer(r, r) / (r @ s)
    return B


class HostMemory:
    """The device memory on the host: W (n x 2M, column major like the kernels'), the state
    block, updated by the library's host copy of the middle-matrix step."""

    def __init__(self, lib, kind, memory, n, init_scale=None, threshold=1e-8):
        self.lib, self.kind, self.M, self.n = lib, kind, memory, n
        self.init = 0.0 if init_scale is None else float(init_scale)
        self.thr = threshold
        R = 2 * memory
        self.W = np.zeros((R, n))
        self.state = np.zeros(lib.ipx_lowrank_state_doubles(memory))
        self.state[0] = self.init if self.init > 0 else 1.0

    def update(self, s, y):
        s, y = np.asarray(s, float), np.asarray(y, float)
        dots = np.concatenate((self.W @ s, self.W @ y, [s @ s, s @ y, y @ y]))
        self.lib.ipx_lowrank_middle_host(self.kind, self.M, self.init, self.thr,
                                         self.state.ctypes.data_as(ctypes.c_void_p),
                                         dots.ctypes.data_as(ctypes.c_void_p))
        if self.state[6] != 0:
            slot = int(self.state[7])
            self.W[slot], self.W[self.M + slot] = s, y

    @property
    def sigma(self):
        return self.state[0]

    @property
    def counts(self):
        return int(self.state[3]), int(self.state[4])

    def C(self):
        R = 2 * self.M
        return self.state[HDR + R * R:HDR + 2 * R * R].reshape(R, R)

    def gram(self):
        R = 2 * self.M
        return self.state[HDR:HDR + R * R].reshape(R, R)

    def B(self):
        return self.sigma * np.eye(self.n) + self.W.T @ self.C() @ self.W

    def dot(self, p):
        return self.sigma * p + self.W.T @ (self.C() @ (self.W @ p))
