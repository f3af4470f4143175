"""Systems, value changes and hierarchy snapshots of the setup-reuse tests (test_setup_reuse_spec.py on the CPU,
test_gpu_setup_reuse.py and its worker on the GPU)."""
import os

import numpy as np
import scipy.sparse as sp

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def system(oc, name):
    """scipy CSR, ascending columns"""
    if name.startswith("lap"):
        stencil, n = (int(x) for x in name[3:].split("_"))
        M = oc.Csr.laplace(n, n, n, stencil)[0].to_scipy().tocsr()
    elif name == "convdiff8":
        from tests.systems import convection_diffusion_3d

        M = convection_diffusion_3d(8).tocsr()
    else:
        g = np.load(os.path.join(GOLD, "random_mmatrix_400.npz"))
        M = sp.csr_matrix((g["data"], g["indices"], g["indptr"]), shape=(400, 400))
    M = M.astype(np.float64)
    M.sort_indices()
    return M


def changed(M, change):
    """the value changes on M's pattern: a unchanged, b8 x 2^-3, b2 x 2, c 3 M + diag(seeded shift in [0, 1]), d every
    off-diagonal entry scaled by a seeded factor in [0.7, 1.3] and the diagonal set to keep the row sums"""
    M = M.copy()
    if change == "a":
        return M
    if change in ("b8", "b2"):
        M.data *= 0.125 if change == "b8" else 2.0
        return M
    coo = M.tocoo()
    if change == "c":
        shift = np.random.default_rng(41).uniform(0.0, 1.0, size=M.shape[0])
        v = 3.0 * coo.data + np.where(coo.row == coo.col, shift[coo.row], 0.0)
    else:
        rowsum = np.asarray(M.sum(axis=1)).ravel()
        f = np.random.default_rng(43).uniform(0.7, 1.3, size=coo.nnz)
        off = coo.row != coo.col
        v = np.where(off, coo.data * f, 0.0)
        offsum = np.bincount(coo.row, weights=v, minlength=M.shape[0])
        v = np.where(off, v, (rowsum - offsum)[coo.row])
    N = sp.csr_matrix((v, (coo.row, coo.col)), shape=M.shape)
    N.sort_indices()
    assert np.array_equal(N.indptr, M.indptr) and np.array_equal(N.indices, M.indices)
    return N


def triples(M):
    coo = M.tocoo()
    return coo.row.astype(np.int64), coo.col.astype(np.int64), np.ascontiguousarray(coo.data, dtype=np.float64)


def snapshot(amg, subs=False):
    """everything the inspection API reports of a hierarchy, level by level"""
    out = []
    nl = amg.num_levels
    for l in range(nl):
        d = {"A": amg.level_csr(l, 0), "norms": amg.level_norms(l), "perm": amg.level_perm(l)}
        if l < nl - 1:
            d["P"], d["R"], d["cf"] = amg.level_csr(l, 2), amg.level_csr(l, 3), amg.level_cf(l)
        if subs:
            d["Az"], d["Ar"] = amg.level_csr(l, 6), amg.level_csr(l, 8)
        out.append(d)
    return out


def same_csr(x, y, values=True):
    return (x[3] == y[3] and np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
            and (not values or np.array_equal(x[2].view(np.int64), y[2].view(np.int64))))


def same_bits(x, y):
    return x.shape == y.shape and np.array_equal(x.view(np.int64), y.view(np.int64))
