"""Restatement of the matrix-matrix extended interpolations (interp_type 16 extended, 17 extended+i; DESIGN.md section 3,
"Matrix-matrix extended interpolation") in plain numpy / scipy, written from the specification's text.  Rows are walked
in stored order (ascending columns), sums are taken one term after the other, nothing is vectorised: the point is to say
the definition a second time, not to be fast."""
import numpy as np
import scipy.sparse as sp

from tests.agg2s_ref import C, F, extended, strength_rows, truncate  # noqa: F401  (strength_rows: for the callers)


def _rows(A):
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A, (lambda i: list(zip(A.indices[A.indptr[i]:A.indptr[i + 1]].tolist(),
                                  A.data[A.indptr[i]:A.indptr[i + 1]].tolist())))


def extended_plus_i(A, strong, m):
    """Type 17 before truncation: list of (coarse columns ascending, weights) per row, and the number of C points.
    Raises ZeroDivisionError naming the row when d_i = 0 meets a non-empty numerator."""
    A, arow = _rows(A)
    n = A.shape[0]
    m = np.asarray(m)
    cidx = -np.ones(n, dtype=int)
    cidx[m == C] = np.arange(int((m == C).sum()))
    sset = [set(int(j) for j in s) for s in strong]
    beta = np.zeros(n)
    for k in range(n):
        b = 0.0
        for l, v in arow(k):
            if l in sset[k] and m[l] == C:
                b += v
        beta[k] = b
    # the right operand: e_k for a C point, the unscaled strong C entries of every other row with beta_k != 0
    right = []
    for k in range(n):
        if m[k] == C:
            right.append([(int(cidx[k]), 1.0)])
        elif beta[k] != 0.0:
            right.append([(int(cidx[l]), v) for l, v in arow(k) if l in sset[k] and m[l] == C])
        else:
            right.append([])
    out = []
    for i in range(n):
        if m[i] == C:
            out.append(([int(cidx[i])], [1.0]))
            continue
        if m[i] != F:
            out.append(([], []))
            continue
        d = 0.0
        left = []  # (k, b_ik), k ascending
        for k, aik in arow(i):
            if k not in sset[i]:
                d += aik  # the diagonal and everything outside S_i
            elif m[k] == C:
                left.append((k, aik))
            elif beta[k] == 0.0:
                d += aik
            else:
                aki = dict(arow(k)).get(i, 0.0)
                delta = beta[k] + aki
                if delta == 0.0:
                    d += aik
                else:
                    bik = aik / delta
                    left.append((k, bik))
                    d += bik * aki
        num = {}
        for k, bik in left:
            for c, w in right[k]:
                num[c] = bik * w if c not in num else num[c] + bik * w
        cols = sorted(num)
        if cols and d == 0.0:
            raise ZeroDivisionError("row %d: zero denominator" % i)
        out.append((cols, [-num[c] / d for c in cols]))
    return out, int((m == C).sum())


def mm_interp(A, strong, m, interp_type, trunc_factor=0.0, pmax=0):
    """P of interp_type 16 / 17 on the marker m as a scipy CSR (n x |C|), explicit zeros kept."""
    rows, nc = (extended if interp_type == 16 else extended_plus_i)(A, strong, m)
    rows = [truncate(c, v, trunc_factor, pmax) for c, v in rows]
    indptr = np.cumsum([0] + [len(c) for c, _ in rows])
    indices = np.array([c for cs, _ in rows for c in cs], dtype=np.int64)
    data = np.array([v for _, vs in rows for v in vs], dtype=np.float64)
    return sp.csr_matrix((data, indices, indptr), shape=(len(rows), nc))
