"""Flow matrices for the aggregate-block and two-level preconditioners: ``A = [G, eps I]`` with G
the node-edge incidence matrix of an N x N grid (m = N^2 balance rows, 2 N (N - 1) flows, N^2
supplies), so that ``A A'`` is the grid's graph Laplacian plus ``eps^2 I``; and the same with 30 %
of the edges removed (many small aggregates, padding inside blocks).
"""
import numpy as np
import scipy.sparse as sps


def grid_edges(N):
    """(tail, head) of the edges of an N x N grid, nodes numbered row by row: the horizontal
    edges row by row, then the vertical ones."""
    node = np.arange(N * N).reshape(N, N)
    tail = np.concatenate((node[:, :-1].ravel(), node[:-1, :].ravel()))
    head = np.concatenate((node[:, 1:].ravel(), node[1:, :].ravel()))
    return tail, head


def flow_matrix(N, eps, keep=None):
    """``[G, eps I]`` as CSR with sorted columns; ``keep``: a boolean mask over the edges."""
    tail, head = grid_edges(N)
    if keep is not None:
        tail, head = tail[keep], head[keep]
    m, e = N * N, len(tail)
    G = sps.csr_matrix((np.concatenate((np.ones(e), -np.ones(e))),
                        (np.concatenate((tail, head)), np.tile(np.arange(e), 2))), shape=(m, e))
    A = sps.hstack((G, eps * sps.identity(m)), format="csr")
    A.sort_indices()
    return A


def grid(N, eps=0.1):
    return flow_matrix(N, eps)


def thinned_grid(N=64, eps=0.1, removed=0.3, seed=1):
    """The grid with ``removed`` of its edges taken out at random."""
    e = 2 * N * (N - 1)
    keep = np.random.default_rng(seed).random(e) >= removed
    return flow_matrix(N, eps, keep)


def rhs(m):
    """The right-hand side of the recorded iteration counts."""
    return np.random.default_rng(0).standard_normal(m)
