"""Restatement of the setup-reuse specification ("Setup reuse") in plain numpy / scipy, sharing no
code with the library: the Galerkin triple product into a given pattern in the contract's order (bits), the same
product by scipy with its error bound (tolerances), the entry lookup through a permutation, the diagonal and the full
l1 norm.  All matrices are scipy CSR with ascending columns."""
import numpy as np
import scipy.sparse as sp


def csr(ia, ja, a, shape):
    return sp.csr_matrix((np.asarray(a, dtype=np.float64), np.asarray(ja), np.asarray(ia)), shape=shape)


def _rows(M):
    ip, ix, dv = M.indptr.tolist(), M.indices.tolist(), M.data.tolist()
    return [list(zip(ix[ip[i]:ip[i + 1]], dv[ip[i]:ip[i + 1]])) for i in range(M.shape[0])]


def triple_product_into_pattern(A, P, pattern):
    """Values of P^T (A P) on the stored entries of `pattern`, by explicit loops: T_kj = sum_m a_km p_mj with m ascending
    along row k, then C_ij = sum_k p_ki T_kj with k ascending; the first product is assigned, the others are added one
    by one (python floats are IEEE doubles, every product and sum is rounded on its own).  Returns (values, fits):
    fits is False when the product's pattern is not the stored one (values is then None)."""
    rows_a, rows_p = _rows(A), _rows(P)
    T = []
    for k in range(A.shape[0]):
        t = {}
        for m, a in rows_a[k]:  # m ascending
            for j, p in rows_p[m]:
                v = a * p
                t[j] = t[j] + v if j in t else v
        T.append(t)
    R = P.T.tocsr()
    R.sort_indices()  # row i of P^T: the fine rows k with p_ki, ascending
    out = np.zeros(pattern.nnz)
    ip, ix = pattern.indptr, pattern.indices
    for i, row in enumerate(_rows(R)):
        acc = {}
        for k, r in row:  # k ascending
            for j, tv in T[k].items():
                v = r * tv
                acc[j] = acc[j] + v if j in acc else v
        cols = ix[ip[i]:ip[i + 1]].tolist()
        if sorted(acc) != cols:
            return None, False
        out[ip[i]:ip[i + 1]] = [acc[j] for j in cols]
    return out, True


def triple_product_scipy(A, P):
    """(P^T A P, |P^T| |A| |P|) by scipy: the product to rounding, and the scale of its entries' error bound."""
    C = (P.T @ (A @ P)).tocsr()
    B = (abs(P).T @ (abs(A) @ abs(P))).tocsr()
    C.sort_indices(), B.sort_indices()
    return C, B


def lookup_through_permutation(A, pattern, rowmap=None, colmap=None):
    """values of the stored entries (r, c) of `pattern`: A[rowmap[r], colmap[c]]; None for an entry A does not store"""
    rows = [dict(r) for r in _rows(A)]
    ip, ix = pattern.indptr, pattern.indices
    out = []
    for r in range(pattern.shape[0]):
        src = rows[r if rowmap is None else int(rowmap[r])]
        for c in ix[ip[r]:ip[r + 1]].tolist():
            out.append(src.get(c if colmap is None else int(colmap[c])))
    return out


def diag_and_l1(A):
    """(diagonal, full l1 norm of the row summed in stored order, carrying the diagonal's sign)"""
    d, l1 = np.zeros(A.shape[0]), np.zeros(A.shape[0])
    for i, row in enumerate(_rows(A)):
        s = 0.0
        for j, v in row:
            s = s + abs(v)
            if j == i:
                d[i] = v
        l1[i] = -s if d[i] < 0 else s
    return d, l1
