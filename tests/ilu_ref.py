"""An independent numpy reference of block-Jacobi ILU(k) on one block, for tests/test_ilu_spec.py and
tests/test_gpu_ilu_irregular.py: the pattern from the level-of-fill definition on a dense level table, the IKJ
factorisation on that pattern, and the exact and the Jacobi application of the factors.

Every numeric part exists twice.  In np.longdouble it is the reference.  In float64, with every product, difference and
quotient rounded on its own and taken in the order of the device kernels (ascending k for an entry's updates, ascending
position for a row's sum), it measures what float64 in that order costs against the reference; the GPU tests take their
tolerance from that distance.  Neither the oracle nor the library is called here, and nothing here merges sorted lists.
"""
import numpy as np
import scipy.sparse as sp

LD = np.longdouble
_INF = np.int32(1 << 20)


def symbolic(A, fill):
    """The ILU(fill) pattern of A as (ia int64, ja int32), columns ascending.  lev = 0 on A's pattern, 'infinite'
    elsewhere; for k ascending, i > k with lev[i,k] <= fill, j > k with lev[k,j] <= fill:
    lev[i,j] = min(lev[i,j], lev[i,k] + lev[k,j] + 1); the entries with lev <= fill are kept."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    lev = np.full((n, n), _INF, dtype=np.int32)
    coo = A.tocoo()
    lev[coo.row, coo.col] = 0
    for k in range(n):
        rows = k + 1 + np.nonzero(lev[k + 1:, k] <= fill)[0]
        cols = k + 1 + np.nonzero(lev[k, k + 1:] <= fill)[0]
        if len(rows) == 0 or len(cols) == 0:
            continue
        prop = lev[rows, k][:, None] + lev[k, cols][None, :] + 1
        sub = lev[np.ix_(rows, cols)]
        lev[np.ix_(rows, cols)] = np.minimum(sub, prop)
    keep = lev <= fill
    ia = np.concatenate(([0], np.cumsum(keep.sum(axis=1)))).astype(np.int64)
    ja = np.nonzero(keep)[1].astype(np.int32)
    return ia, ja


def level_sets(ia, ja):
    """(lower, upper): the number of level sets of the strict lower and of the strict upper triangle of the pattern
    (the longest dependency chain, counted in rows)."""
    n = len(ia) - 1
    ll = np.zeros(n, dtype=np.int64)
    lu = np.zeros(n, dtype=np.int64)
    for i in range(n):
        c = ja[ia[i]:ia[i + 1]]
        c = c[c < i]
        if len(c):
            ll[i] = ll[c].max() + 1
    for i in range(n - 1, -1, -1):
        c = ja[ia[i]:ia[i + 1]]
        c = c[c > i]
        if len(c):
            lu[i] = lu[c].max() + 1
    return (int(ll.max()) + 1, int(lu.max()) + 1) if n else (0, 0)


def _seq_sub(s, prods):
    """((s - p0) - p1) - ..., every difference rounded on its own"""
    if len(prods) == 0:
        return s
    return np.subtract.accumulate(np.concatenate(([s], prods)))[-1]


class Factors:
    """L (unit diagonal not stored) and U of the IKJ factorisation on a pattern, as one CSR in `dtype`."""

    def __init__(self, A, fill, dtype, pattern=None):
        A = sp.csr_matrix(A).astype(np.float64)
        A.sort_indices()
        n = A.shape[0]
        ia, ja = symbolic(A, fill) if pattern is None else pattern
        self.n, self.ia, self.ja, self.dtype = n, ia, ja, dtype
        row = np.repeat(np.arange(n), np.diff(ia))
        d = np.nonzero(row == ja)[0]
        assert len(d) == n, "every row needs a stored diagonal"
        self.dpos = d.astype(np.int64)
        # A's values on A's positions, zero on the fill
        v = np.zeros(len(ja), dtype=dtype)
        for i in range(n):
            where = dict(zip(ja[ia[i]:ia[i + 1]].tolist(), range(ia[i], ia[i + 1])))
            for q in range(A.indptr[i], A.indptr[i + 1]):
                v[where[int(A.indices[q])]] = A.data[q]
        self.a0 = v.copy()
        # IKJ: for k < i in row i, ascending: l_ik = a_ik / u_kk;  a_ij -= l_ik u_kj  for j > k in both rows
        w = np.zeros(n, dtype=dtype)
        mark = np.full(n, -1, dtype=np.int64)
        for i in range(n):
            lo, hi = ia[i], ia[i + 1]
            cols = ja[lo:hi]
            w[cols] = v[lo:hi]
            mark[cols] = i
            for k in cols[cols < i]:
                l = w[k] / v[self.dpos[k]]
                w[k] = l
                ulo, uhi = self.dpos[k] + 1, ia[k + 1]
                kc = ja[ulo:uhi]
                hit = mark[kc] == i
                J = kc[hit]
                w[J] = w[J] - l * v[ulo:uhi][hit]
            v[lo:hi] = w[cols]
        self.a = v
        self.nlower = (self.dpos - ia[:-1]).astype(np.int64)
        self.nupper = (ia[1:] - self.dpos - 1).astype(np.int64)

    def csr(self):
        return sp.csr_matrix((self.a.astype(np.float64), self.ja, self.ia), shape=(self.n, self.n))

    def dense_LU(self):
        """(L with its unit diagonal, U) as dense arrays in self.dtype"""
        F = np.zeros((self.n, self.n), dtype=self.dtype)
        row = np.repeat(np.arange(self.n), np.diff(self.ia))
        F[row, self.ja] = self.a
        return np.tril(F, -1) + np.eye(self.n, dtype=self.dtype), np.triu(F)

    def apply_exact(self, r):
        """z = U^-1 L^-1 r by forward and backward substitution"""
        ia, ja, a, n = self.ia, self.ja, self.a, self.n
        r = np.asarray(r, dtype=self.dtype)
        y = np.zeros(n, dtype=self.dtype)
        z = np.zeros(n, dtype=self.dtype)
        for i in range(n):
            lo, d = ia[i], self.dpos[i]
            y[i] = _seq_sub(r[i], a[lo:d] * y[ja[lo:d]])
        for i in range(n - 1, -1, -1):
            d, hi = self.dpos[i], ia[i + 1]
            z[i] = _seq_sub(y[i], a[d + 1:hi] * z[ja[d + 1:hi]]) / a[d]
        return z

    def _sweep(self, first, count, rhs, x):
        """s_i = rhs_i - sum over the row's `count[i]` entries from position first[i], in ascending position"""
        s = rhs.copy()
        for p in range(int(count.max()) if len(count) else 0):
            rows = np.nonzero(count > p)[0]
            pos = first[rows] + p
            s[rows] = s[rows] - self.a[pos] * x[self.ja[pos]]
        return s

    def apply_jacobi(self, r, lower_it, upper_it):
        """y <- r - L_strict y, lower_it times from y = r;  z <- D^-1 (y - U_strict z), upper_it times from D^-1 y"""
        r = np.asarray(r, dtype=self.dtype)
        d = self.a[self.dpos]
        y = r.copy()
        for _ in range(lower_it):
            y = self._sweep(self.ia[:-1], self.nlower, r, y)
        z = y / d
        for _ in range(upper_it):
            z = self._sweep(self.dpos + 1, self.nupper, y, z) / d
        return z


def richardson(A, F, b, max_iter, tol, ncomp=1, jacobi=None):
    """x += M^-1 (b - A x) from x = 0 in float64, the order of the library's ILU solver: the residual of every
    component first, one norm over all of them (numpy), the test  ||r|| / ||b|| <= tol  before each update, the
    preconditioner applied per component.  b has shape (ncomp, n).  Returns (x, iterations, rel of every test)."""
    A = sp.csr_matrix(A)
    b = np.asarray(b, dtype=np.float64).reshape(ncomp, -1)
    x = np.zeros_like(b)
    bn = np.sqrt(np.sum(b * b))
    it, rels = 0, []
    while it < max_iter:
        r = np.stack([b[c] - A @ x[c] for c in range(ncomp)])
        rn = np.sqrt(np.sum(r * r))
        rels.append(rn / bn if bn > 0 else rn)
        if rels[-1] <= tol:
            break
        for c in range(ncomp):
            x[c] = x[c] + (F.apply_exact(r[c]) if jacobi is None else F.apply_jacobi(r[c], *jacobi))
        it += 1
    return x, it, rels


def deviation(f64, ref):
    """max|f64 - ref| in longdouble, as a float"""
    return float(np.abs(np.asarray(f64, dtype=LD) - np.asarray(ref, dtype=LD)).max()) if len(ref) else 0.0


def bound(f64, ref):
    """The tolerance of the GPU tests on a device result against the longdouble reference `ref`: 4 times the distance
    of the float64 restatement `f64` from it (a device division may round differently) plus 2 eps max|ref|."""
    top = float(np.abs(np.asarray(ref, dtype=LD)).max()) if len(ref) else 0.0
    return 4.0 * deviation(f64, ref) + 2.0 * np.finfo(np.float64).eps * top
