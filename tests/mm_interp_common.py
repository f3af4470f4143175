"""Helpers shared by the CPU and GPU tests of the matrix-matrix extended interpolation (interp_type 16 / 17) and by
profiles/mm_interp_measure.py: the test operators beyond tests/agg2s_common.py, levels in their natural numbering, the
comparison with the restatement of tests/mm_interp_ref.py."""
import numpy as np
import scipy.sparse as sp

from tests import mm_interp_ref as ref
from tests.agg2s_common import csr

THETA = 0.57  # strong_threshold of mi.BoomerAMG's defaults (the app's)


def upwind_convection(n=9, v=(1.0, 0.5, 0.25)):
    """7-point Laplacian on n^3 plus first-order upwind convection with velocity v (in units of 1 / h): the upstream
    neighbour of every direction takes -v_d more, the diagonal v_d.  Nonsymmetric, still an M-matrix."""
    def lap1(k):
        return sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(k, k))

    def up1(k):
        return sp.diags([-1.0, 1.0], [-1, 0], shape=(k, k))
    I = sp.identity(n)
    M = sp.kron(sp.kron(I, I), lap1(n) + v[0] * up1(n)) + sp.kron(sp.kron(I, lap1(n) + v[1] * up1(n)), I) \
        + sp.kron(sp.kron(lap1(n) + v[2] * up1(n), I), I)
    M = M.tocsr()
    M.sort_indices()
    return M


def one_directional(n=300):
    """Row i stores the diagonal and the columns i + 1, i + 2 (strong: -1, -0.9), i + 5 (weak: -0.5) and i + 9 (strong:
    -0.8) where they exist: no pair (i, k), (k, i) is stored both ways, so a_ki = 0 for every strong neighbour k of i."""
    M = sp.lil_matrix((n, n))
    for i in range(n):
        M[i, i] = 3.5
        for o, v in ((1, -1.0), (2, -0.9), (5, -0.5), (9, -0.8)):
            if i + o < n:
                M[i, i + o] = v
    M = M.tocsr()
    M.sort_indices()
    return M


def strength_csr(A, theta=THETA):
    rows = ref.strength_rows(A, theta)
    indptr = np.cumsum([0] + [len(r) for r in rows])
    indices = np.concatenate(rows) if len(rows) and indptr[-1] else np.zeros(0, dtype=int)
    return rows, sp.csr_matrix((np.ones(indptr[-1]), indices.astype(np.int64), indptr), shape=A.shape)


def permute_keep_zeros(P, row_new_of_old, col_old_of_new):
    """rows: natural row i = reported row row_new_of_old[i]; columns: reported column q = natural column
    col_old_of_new[q]; explicit zeros survive (the arrays are handled, not scipy's arithmetic)"""
    indptr, indices, data = [0], [], []
    for i in range(P.shape[0]):
        r = row_new_of_old[i]
        c = col_old_of_new[P.indices[P.indptr[r]:P.indptr[r + 1]]]
        v = P.data[P.indptr[r]:P.indptr[r + 1]]
        o = np.argsort(c, kind="stable")
        indices += list(c[o])
        data += list(v[o])
        indptr.append(len(indices))
    return sp.csr_matrix((np.array(data, dtype=float), np.array(indices, dtype=np.int64), np.array(indptr)), shape=P.shape)


def natural_level(amg, l):
    """A of level l, the marker handed on and P in the level's NATURAL numbering (the one the hierarchy is built in: the
    specification's "stored order"; level_csr reports C-first renumbered copies)"""
    perm = amg.level_perm(l).astype(np.int64)       # perm[new] = old
    permc = amg.level_perm(l + 1).astype(np.int64)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    A = csr(amg, l, 0)[inv][:, inv].tocsr()
    A.sort_indices()
    cf = np.empty(len(perm), dtype=np.int64)
    cf[perm] = amg.level_cf(l)
    return A, cf, permute_keep_zeros(csr(amg, l, 2), inv, permc)


def marker_before_interpolation(cf, strong):
    """PMIS marks exactly the points without a strong neighbour special (-3); the interpolation hands them on as F"""
    m = np.array(cf, dtype=np.int64)
    for i, s in enumerate(strong):
        if len(s) == 0:
            assert m[i] == -1
            m[i] = -3
    return m


def same_pattern_close_values(P, Q, rtol=1e-13):
    assert P.shape == Q.shape, (P.shape, Q.shape)
    assert np.array_equal(P.indptr, Q.indptr) and np.array_equal(P.indices, Q.indices), "patterns differ"
    err = np.abs(P.data - Q.data)
    print("max relative difference %.3e over %d entries" % ((err / np.maximum(np.abs(Q.data), 1e-300)).max(initial=0.0), len(err)))
    assert np.all(err <= rtol * np.abs(Q.data))


def as_csr(parts):
    ia, ja, a, shape = parts
    return sp.csr_matrix((a, ja, ia), shape=shape)
