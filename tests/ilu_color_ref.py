"""Python reference of the multicolour ordering of the ILU (local_reordering 2; DESIGN.md section 3, "Multicolour
ordering"), for tests/test_ilu_color_spec.py and tests/test_gpu_ilu_color.py.  It states the result, not the rounds:
the first-fit greedy colouring of the graph of D + D^T (no diagonal) with the rows taken in priority order, the
ordering by (colour, index), and the number of Jones-Plassmann rounds as the longest path of decreasing priority.
Nothing here calls the library."""
import numpy as np
import scipy.sparse as sp


def fmix32(h):
    """The MurmurHash3 32-bit finaliser on uint32 (scalars or arrays)."""
    h = np.asarray(h, dtype=np.uint64) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h.astype(np.uint32)


def weights(n):
    """w(i) = fmix32(uint32(i) + 1)"""
    return fmix32(np.arange(n, dtype=np.uint64) + 1)


def priority_order(n):
    """The rows in priority order: larger weight first, the smaller index first among equal weights."""
    w = weights(n).astype(np.int64)
    return np.lexsort((np.arange(n), -w))


def graph(D):
    """The pattern of D + D^T without the diagonal as CSR (stored entries count, whatever their value)."""
    D = sp.csr_matrix(D)
    n = D.shape[0]
    S = sp.csr_matrix((np.ones(D.nnz), D.indices, D.indptr), shape=(n, n))
    S = sp.csr_matrix(S + S.T)
    S.setdiag(0)
    S.eliminate_zeros()
    S.sort_indices()
    return S


class Ordering:
    """colour (by row), ncolours, perm (row q of the reordered block is row perm[q]), rounds."""

    def __init__(self, D):
        G = graph(D)
        n = G.shape[0]
        order = priority_order(n)
        rank = np.empty(n, dtype=np.int64)  # position in priority order
        rank[order] = np.arange(n)
        colour = np.full(n, -1, dtype=np.int32)
        rnd = np.zeros(n, dtype=np.int64)  # the round that colours the row
        for i in order:
            nb = G.indices[G.indptr[i]:G.indptr[i + 1]]
            before = nb[rank[nb] < rank[i]]
            taken = set(colour[before].tolist())
            c = 0
            while c in taken:
                c += 1
            colour[i] = c
            rnd[i] = 1 + (rnd[before].max() if len(before) else 0)
        self.n, self.G = n, G
        self.colour = colour
        self.ncolours = int(colour.max()) + 1 if n else 0
        self.rounds = int(rnd.max()) if n else 0
        self.perm = np.lexsort((np.arange(n), colour)).astype(np.int32)
        self.max_degree = int(np.diff(G.indptr).max()) if n else 0

    def permuted(self, D):
        """B = P D P^T with ascending columns"""
        B = sp.csr_matrix(D)[self.perm][:, self.perm].tocsr()
        B.sort_indices()
        return B
