"""Helpers shared by the CPU and GPU tests of the two-stage extended interpolation (agg_interp_type 5) and by
profiles/agg2s_two_grid.py: host-only assembly and setup through the C ABI, the test operators, the two-grid factor."""
import os

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def ij_host(mi, M):
    """an assembled single-rank IJ matrix without touching the device"""
    M = sp.csr_matrix(M)
    n = M.shape[0]
    A = mi.IJMatrix.__new__(mi.IJMatrix)
    A.h = mi.vp()
    mi.call("HYPRE_IJMatrixCreate", 0, mi.c_big(0), mi.c_big(n - 1), mi.c_big(0), mi.c_big(n - 1), mi.C.byref(A.h))
    A.par = mi.vp()
    mi.call("HYPRE_IJMatrixGetObject", A.h, mi.C.byref(A.par))
    coo = M.tocoo()
    A.set_values_coo(coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data.astype(np.float64))
    mi.call("HYPRE_MI_IJMatrixAssembleHostOnly", A.h)
    return A


def host_amg(mi, A, **kw):
    """host-only setup; the stage markers of type-5 levels are kept for level_agg_markers()"""
    amg = mi.BoomerAMG(print_level=0, keep_agg_markers=1, **kw)
    mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
    return amg


def csr(amg, level, which):
    ia, ja, a, shape = amg.level_csr(level, which)
    return sp.csr_matrix((a, ja, ia), shape=shape)


def random_mmatrix():
    g = np.load(os.path.join(GOLD, "random_mmatrix_400.npz"))
    n = len(g["indptr"]) - 1
    return sp.csr_matrix((g["data"], g["indices"], g["indptr"]), shape=(n, n))


def anisotropic(n=9, eps=0.05):
    """-eps u_xx - u_yy - u_zz on an n^3 grid, Dirichlet on the x = 0 face only (natural boundaries elsewhere): the x
    neighbours are weak at theta = 0.57, and away from that face every row sums to zero."""
    def lap1(k, dirichlet_left):
        T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(k, k)).tolil()
        T[k - 1, k - 1] = 1.0
        if not dirichlet_left:
            T[0, 0] = 1.0
        return T.tocsr()
    I = sp.identity(n)
    M = (eps * sp.kron(sp.kron(I, I), lap1(n, True)) + sp.kron(sp.kron(I, lap1(n, False)), I)
         + sp.kron(sp.kron(lap1(n, False), I), I)).tocsr()
    M.sort_indices()
    return M


def zero_denominator_matrix(n=60):
    """Circulant rows: one strong neighbour (-1 at i + 1), four weak ones (-0.5 each, not below 0.57 * -1) and the
    diagonal 2 that cancels them, so every F row has d_i = 2 - 4 * 0.5 = 0 and the numerator -1 * M_(i+1); the row sum
    -1 stays within max_row_sum * 2."""
    M = sp.lil_matrix((n, n))
    for i in range(n):
        M[i, i] = 2.0
        M[i, (i + 1) % n] = -1.0
        for o in (-1, 2, -2, 3):
            M[i, (i + o) % n] = -0.5
    return M.tocsr()


def two_grid_factor(A, P):
    """spectral radius of S (I - P (P^T A P)^-1 P^T A) S with S = one symmetric Gauss-Seidel sweep (dense algebra):
    the figure of profiles/r03_two_grid_aggressive.txt"""
    Ad, Pd = A.toarray(), P.toarray()
    I = np.eye(Ad.shape[0])
    Ssym = (I - np.linalg.solve(np.triu(Ad), Ad)) @ (I - np.linalg.solve(np.tril(Ad), Ad))
    K = I - Pd @ np.linalg.solve(Pd.T @ Ad @ Pd, Pd.T @ Ad)
    return float(np.abs(np.linalg.eigvals(Ssym @ K @ Ssym)).max())
