"""numpy restatement of the multicolour Gauss-Seidel smoother (relax types 40 / 41 / 42): exact
Gauss-Seidel by sequential substitution in the stored row order, and the validity check of a colouring."""
import numpy as np
import scipy.sparse as sp

FORWARD, BACKWARD, SYMMETRIC = 40, 41, 42


def _pass(indptr, indices, data, diag, u, f, omega, rows):
    for i in rows:
        s = slice(indptr[i], indptr[i + 1])
        u[i] = u[i] + omega * (f[i] - np.dot(data[s], u[indices[s]])) / diag[i]


def sweep(A, u, f, omega=1.0, direction=FORWARD, dtype=np.float64, order=None):
    """u_i <- u_i + omega (f_i - sum_j a_ij u_j) / a_ii, row after row, u read in place: the rows in stored order
    (direction 40), in reverse order (41), or one after the other (42).  order: another row sequence for the forward
    pass (its reverse for the backward one).  dtype float64 or np.longdouble: the arithmetic of the whole sweep."""
    A = sp.csr_matrix(A)
    A.sort_indices()
    n = A.shape[0]
    data, diag = A.data.astype(dtype), A.diagonal().astype(dtype)
    u, f, omega = np.array(u, dtype=dtype), np.asarray(f, dtype=dtype), dtype(omega)
    rows = np.arange(n) if order is None else np.asarray(order)
    assert direction in (FORWARD, BACKWARD, SYMMETRIC)
    if direction in (FORWARD, SYMMETRIC):
        _pass(A.indptr, A.indices, data, diag, u, f, omega, rows)
    if direction in (BACKWARD, SYMMETRIC):
        _pass(A.indptr, A.indices, data, diag, u, f, omega, rows[::-1])
    return u


def jacobi(A, u, f, omega=1.0):
    A = sp.csr_matrix(A)
    return u + omega * (f - A @ u) / A.diagonal()


def colouring_conflicts(A, colour):
    """the stored entries (i, j), i != j, of A or of its transpose whose rows have the same colour"""
    C = sp.coo_matrix(A)
    off = C.row != C.col
    r, c = C.row[off], C.col[off]
    colour = np.asarray(colour)
    bad = colour[r] == colour[c]
    return list(zip(r[bad].tolist(), c[bad].tolist()))


def colour_ranges(colour, nc):
    """number of maximal runs of equal colour in [0, nc) and in [nc, n)"""
    def runs(c):
        return 0 if len(c) == 0 else 1 + int((np.diff(c) != 0).sum())
    colour = np.asarray(colour)
    return runs(colour[:nc]), runs(colour[nc:])


def max_degree(A):
    """the largest number of neighbours of a row in the graph of A + A^T without the diagonal"""
    A = sp.csr_matrix(A)
    S = (abs(A) + abs(A).T).tocsr()
    S.data[:] = 1.0
    S = (S - sp.diags(S.diagonal())).tocsr()
    S.eliminate_zeros()
    return int(np.diff(S.indptr).max()) if S.shape[0] else 0
