"""numpy restatement of the iterative ILU(0) setup ("Iterative ILU(0) setup") and an exact
ILU(0), for tests/test_itilu_spec.py and tests/test_gpu_itilu.py.

Values are kept in the CSR order of the pattern S of A (columns ascending, the diagonal stored): x[e] is l_ij for an
entry e = (i, j) with i > j and u_ij for i <= j.  One synchronous sweep is, for every entry,
    s = a_ij; s -= l_ik * u_kj  (k < min(i, j) with (i,k), (k,j) in S, ascending k); l_ij = s / u_jj  or  u_ij = s
with every product and difference rounded on its own -- what the device computes without fused multiply-add."""
import numpy as np
import scipy.sparse as sp


class Plan:
    """The pattern of A and, for every stored entry, its (l_ik, u_kj) position pairs in ascending k."""

    def __init__(self, A):
        A = sp.csr_matrix(A).copy()
        A.sort_indices()
        self.A = A
        n = A.shape[0]
        ia, ja = A.indptr, A.indices
        self.a = A.data.astype(np.float64).copy()
        self.row = np.repeat(np.arange(n), np.diff(ia))
        self.col = ja.astype(np.int64)
        dpos = np.full(n, -1, dtype=np.int64)
        diag = self.row == self.col
        dpos[self.row[diag]] = np.nonzero(diag)[0]
        assert (dpos >= 0).all(), "every row needs a stored diagonal"
        self.dpos = dpos
        self.lower = self.row > self.col
        self.dcol = dpos[self.col]  # position of u_jj (used for the L entries)
        where = [dict(zip(ja[ia[i]:ia[i + 1]].tolist(), range(ia[i], ia[i + 1]))) for i in range(n)]
        pairs = []
        for e in range(len(ja)):
            i, j = int(self.row[e]), int(self.col[e])
            m = min(i, j)
            lst = []
            for kk in range(ia[i], ia[i + 1]):
                k = int(ja[kk])
                if k >= m:
                    break
                q = where[k].get(j)
                if q is not None:
                    lst.append((kk, q))
            pairs.append(lst)
        self.npairs = np.array([len(p) for p in pairs], dtype=np.int64)
        width = int(self.npairs.max()) if len(pairs) else 0
        self.pl = np.zeros((len(pairs), width), dtype=np.int64)
        self.pu = np.zeros((len(pairs), width), dtype=np.int64)
        for e, lst in enumerate(pairs):
            for p, (kk, q) in enumerate(lst):
                self.pl[e, p], self.pu[e, p] = kk, q

    def start(self):
        """x_0: L = the strictly lower part of A, column j divided by a_jj; U = the upper part of A."""
        x = self.a.copy()
        lo = self.lower
        x[lo] = self.a[lo] / self.a[self.dcol[lo]]
        return x

    def _sums(self, x):
        s = self.a.copy()
        for p in range(self.pl.shape[1]):
            e = np.nonzero(self.npairs > p)[0]
            s[e] = s[e] - x[self.pl[e, p]] * x[self.pu[e, p]]
        return s

    def sweep(self, x):
        """one synchronous sweep (types 3 and 4): reads only x"""
        s = self._sums(x)
        lo = self.lower
        s[lo] = s[lo] / x[self.dcol[lo]]
        return s

    def correction(self, x_old, x_new):
        """c = max|x_new - x_old| / max|x_new|"""
        xm = np.abs(x_new).max()
        d = np.abs(x_new - x_old).max()
        return d / xm if xm > 0 else d

    def residual(self, x):
        """rho = max over S of |a_ij - (L U)_ij| / max|a_ij|"""
        s = self._sums(x)
        lo = self.lower
        t = x.copy()
        t[lo] = x[lo] * x[self.dcol[lo]]
        s = s - t
        am = np.abs(self.a).max()
        return np.abs(s).max() / am if am > 0 else np.abs(s).max()

    def run(self, sweeps):
        x = self.start()
        for _ in range(sweeps):
            x = self.sweep(x)
        return x

    def stop_sweep(self, tol, max_iter):
        """the sweep after which option bit 2 stops (the first with c <= tol), or max_iter"""
        x = self.start()
        for m in range(1, max_iter + 1):
            xn = self.sweep(x)
            c = self.correction(x, xn)
            x = xn
            if c <= tol:
                return m
        return max_iter

    def csr(self, x):
        return sp.csr_matrix((x, self.A.indices, self.A.indptr), shape=self.A.shape)


def exact_ilu0(A):
    """ILU(0) by the IKJ loop (the order of the library's level-scheduled factorisation): values in A's CSR order."""
    A = sp.csr_matrix(A).copy()
    A.sort_indices()
    n = A.shape[0]
    ia, ja = A.indptr, A.indices
    v = A.data.astype(np.float64).copy()
    dpos = np.full(n, -1, dtype=np.int64)
    where = [dict(zip(ja[ia[i]:ia[i + 1]].tolist(), range(ia[i], ia[i + 1]))) for i in range(n)]
    for i in range(n):
        dpos[i] = where[i].get(i, -1)
    for i in range(n):
        for kk in range(ia[i], ia[i + 1]):
            k = int(ja[kk])
            if k >= i:
                break
            l = v[kk] / v[dpos[k]]
            v[kk] = l
            for jj in range(kk + 1, ia[i + 1]):
                q = where[k].get(int(ja[jj]))
                if q is not None:
                    v[jj] = v[jj] - l * v[q]
    return v


def laplace(n, stencil=7):
    """the 3-D Laplacian of the library's build_laplace_system (7 or 27 points), natural order"""
    if stencil == 7:
        T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n))
        I = sp.identity(n)
        return (sp.kron(sp.kron(I, I), T) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(T, I), I)).tocsr()
    B = sp.diags([1.0, 1.0, 1.0], [-1, 0, 1], shape=(n, n))
    M = sp.kron(sp.kron(B, B), B).tocsr()
    M = -M
    M.setdiag(26.0)
    return M.tocsr()


def nonsymmetric(n=800, seed=5):
    """a seeded nonsymmetric, strictly diagonally dominant matrix with a ragged pattern"""
    rng = np.random.default_rng(seed)
    M = sp.random(n, n, density=8.0 / n, random_state=rng, format="csr")
    M.data = rng.uniform(-1.0, 1.0, size=M.data.shape)
    M.setdiag(0.0)
    M.eliminate_zeros()
    d = np.abs(M).sum(axis=1).A1 * 1.5 + 1.0
    return (M + sp.diags(d)).tocsr()
