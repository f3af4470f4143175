"""Restatement of the two-stage extended interpolation of aggressive levels (agg_interp_type 5; DESIGN.md section 3,
"Two-stage extended interpolation") in plain numpy / scipy, written from the specification's text.  Rows are walked
in stored order (ascending columns), sums are taken one term after the other, nothing is vectorised: the point is to
say the definition a second time, not to be fast."""
import numpy as np
import scipy.sparse as sp

C, F, SF = 1, -1, -3


def strength_rows(A, theta, max_row_sum=0.9):
    """Strong neighbours of every row (ascending): j != i with a_ij < theta * min(0, min_k a_ik) for a_ii >= 0
    (mirrored for a_ii < 0); rows with |sum_j a_ij| > max_row_sum |a_ii| have none."""
    A = sp.csr_matrix(A)
    A.sort_indices()
    out = []
    for i in range(A.shape[0]):
        cols = A.indices[A.indptr[i]:A.indptr[i + 1]]
        vals = A.data[A.indptr[i]:A.indptr[i + 1]]
        diag = float(vals[cols == i].sum())
        off = cols != i
        if max_row_sum < 1.0 and abs(vals.sum()) > abs(diag) * max_row_sum or not off.any():
            out.append(np.zeros(0, dtype=int))
            continue
        if diag < 0:
            thr = theta * max(0.0, vals[off].max())
            out.append(cols[off & (vals > thr)].astype(int))
        else:
            thr = theta * min(0.0, vals[off].min())
            out.append(cols[off & (vals < thr)].astype(int))
    return out


def truncate(cols, vals, trunc_factor, pmax):
    """|p| descending, position ascending; rescaled to the row sum; the kept entries stay in their order."""
    if len(vals) == 0 or (trunc_factor <= 0.0 and pmax <= 0):
        return list(cols), list(vals)
    total = 0.0
    for v in vals:
        total += v
    big = max(abs(v) for v in vals)
    keep = [k for k in range(len(vals)) if trunc_factor <= 0.0 or abs(vals[k]) >= trunc_factor * big]
    if pmax > 0 and len(keep) > pmax:
        ranked = sorted(keep, key=lambda k: (-abs(vals[k]), k))
        keep = sorted(ranked[:pmax])
    kept = 0.0
    for k in keep:
        kept += vals[k]
    scale = total / kept if kept != 0.0 else 1.0
    return [cols[k] for k in keep], [vals[k] * scale for k in keep]


def extended(A, strong, m, rows=None):
    """E(A, S, m): list of (coarse columns ascending, weights) for the rows asked for (default: all), and the number
    of C points of m.  Raises ZeroDivisionError naming the row when d_i = 0 meets a non-empty numerator."""
    A = sp.csr_matrix(A)
    A.sort_indices()
    n = A.shape[0]
    m = np.asarray(m)
    cidx = -np.ones(n, dtype=int)
    cidx[m == C] = np.arange(int((m == C).sum()))
    arow = lambda i: zip(A.indices[A.indptr[i]:A.indptr[i + 1]], A.data[A.indptr[i]:A.indptr[i + 1]])
    sset = [set(int(j) for j in s) for s in strong]
    beta = np.zeros(n)
    for k in range(n):
        b = 0.0
        for l, v in arow(k):
            if l in sset[k] and m[l] == C:
                b += v
        beta[k] = b
    out = []
    for i in (range(n) if rows is None else rows):
        if m[i] == C:
            out.append(([int(cidx[i])], [1.0]))
            continue
        if m[i] != F:
            out.append(([], []))
            continue
        d = 0.0
        num = {}
        for k, aik in arow(i):
            if k not in sset[i]:
                d += aik  # the diagonal and the weak entries
                continue
            if m[k] == C:
                terms = [(int(cidx[k]), 1.0)]
            elif beta[k] != 0.0:
                terms = [(int(cidx[l]), akl / beta[k]) for l, akl in arow(k) if l in sset[k] and m[l] == C]
            else:
                d += aik
                terms = []
            for c, w in terms:
                num[c] = aik * w if c not in num else num[c] + aik * w
        cols = sorted(num)
        if cols and d == 0.0:
            raise ZeroDivisionError("row %d: zero denominator" % i)
        out.append((cols, [-num[c] / d for c in cols]))
    return out, int((m == C).sum())


def _csr(rows, ncols):
    indptr = np.cumsum([0] + [len(c) for c, _ in rows])
    indices = np.array([c for cs, _ in rows for c in cs], dtype=np.int64)
    data = np.array([v for _, vs in rows for v in vs], dtype=np.float64)
    return sp.csr_matrix((data, indices, indptr), shape=(len(rows), ncols))


def product_rows(P1, P2):
    """rows of P1 * P2: entry (i, j) = sum over the stored order of P1's row i, first product assigned, the others
    added one by one; columns ascending; an entry that cancels to zero stays"""
    out = []
    for cols, vals in P1:
        acc = {}
        for k, v in zip(cols, vals):
            for c, w in zip(*P2[k]):
                acc[c] = v * w if c not in acc else acc[c] + v * w
        cs = sorted(acc)
        out.append((cs, [acc[c] for c in cs]))
    return out


def two_stage(A, strong, m1, m2, p12_trunc_factor=0.0, p12_max=0, trunc_factor=0.0, pmax=0, parts=False):
    """P = trunc(trunc12(E(A, S, m1)) * trunc12(C1 rows of E(A, S, m2))) as a scipy CSR (n x |C2|), explicit zeros kept."""
    m1, m2 = np.asarray(m1), np.asarray(m2)
    c1 = np.flatnonzero(m1 == C)
    assert np.all(m1[m2 == C] == C), "C2 must lie inside C1"
    P1, nc1 = extended(A, strong, m1)
    P2, nc2 = extended(A, strong, m2, rows=c1)
    P1 = [truncate(c, v, p12_trunc_factor, p12_max) for c, v in P1]
    P2 = [truncate(c, v, p12_trunc_factor, p12_max) for c, v in P2]
    P = [truncate(c, v, trunc_factor, pmax) for c, v in product_rows(P1, P2)]
    if parts:
        return _csr(P, nc2), _csr(P1, nc1), _csr(P2, nc2)
    return _csr(P, nc2)
