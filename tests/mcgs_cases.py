"""Operators of the multicolour Gauss-Seidel tests (tests/test_mcgs_spec.py, tests/test_gpu_mcgs.py): the smallest
shapes at which the colouring, the (block, colour) sort or the in-place pass can go wrong.  Every generator is seeded."""
import numpy as np
import scipy.sparse as sp

from tests import air_cases
from tests import dict_cases
from tests import systems


def laplace(n, stencil):
    """the driver's n^3 Laplacian: 7-point (diag 6, off -1) or 27-point (diag 26, off -1), lexicographic numbering"""
    T = sp.diags([1.0, 1.0, 1.0], [-1, 0, 1], shape=(n, n))
    I = sp.identity(n)
    if stencil == 7:
        K = sp.diags([1.0, 1.0], [-1, 1], shape=(n, n))
        B = sp.kron(sp.kron(I, I), K) + sp.kron(sp.kron(I, K), I) + sp.kron(sp.kron(K, I), I)
        M = (6.0 * sp.identity(n ** 3) - B).tocsr()
    else:
        B = sp.kron(sp.kron(T, T), T)
        M = (27.0 * sp.identity(n ** 3) - B).tocsr()
    M.sort_indices()
    return M


def unsymmetric_pattern(n=900, seed=21):
    """rows that store (i, j) without (j, i): a one-way random pattern (systems.mixed_sign_system without the
    symmetrisation), so that colouring the pattern of D alone would give two coupled rows one colour"""
    M = systems.mixed_sign_system(n, seed, .2, .2, 4.0, symmetric_pattern=False)
    P = M.copy()
    P.data[:] = 1.0
    one_way = (P - P.multiply(P.T)).nnz
    assert one_way > n  # most couplings are stored on one side only
    return M


def diagonal(n=50):
    return sp.diags(np.linspace(1.0, 3.0, n)).tocsr()


def wide(n=263, per=60, seed=8):
    """about 2 * per entries per row: the operator gets the wide (4096-entry) tiles, its colouring dozens of colours with
    ranges of one, two, three rows"""
    M = systems.mixed_sign_system(n, seed, .3, .25, per)
    assert M.nnz / n >= 100.0
    return M


def long_row(n=2309, length=2100, seed=13):
    """one row with more entries than a tile holds (2048), stored on one side only, in an otherwise sparse operator"""
    rng = np.random.default_rng(seed)
    M = systems.mixed_sign_system(n, seed, 0.0, 0.2, 2.0).tolil()
    h = 1157
    cols = rng.choice(np.setdiff1d(np.arange(n), [h]), size=length, replace=False)
    M[h, cols] = -1.0
    M[h, h] = 1.01 * length
    M = M.tocsr()
    M.sort_indices()
    assert M.indptr[h + 1] - M.indptr[h] > 2048
    return M


def hub(seed=3):
    """an irregular operator with hub rows of 100 and more entries (systems.hub_system)"""
    M, hubs, lengths = systems.hub_system((100, 129, 180), seed, base=(1100, 49, .3, .25, 4.5))
    return M


def many_values(n=2000, seed=58):
    """more than 65536 entries and far more than 256 distinct values: the operator keeps the plain value stream"""
    M = systems.mixed_sign_system(n, seed, .5, .3, 18)
    assert M.nnz >= dict_cases.THRESHOLD and dict_cases.distinct(M) > 256
    return M


def constant_stencil(n=15):
    """27-point, 15^3: more than 65536 entries with two distinct values, so level 0 gets the value dictionary"""
    M = laplace(n, 27)
    assert M.nnz >= dict_cases.THRESHOLD and dict_cases.distinct(M) <= 256
    return M


CASES = {
    "lap7_6": lambda: laplace(6, 7),
    "lap27_6": lambda: laplace(6, 27),
    "mixed700": lambda: systems.mixed_sign_system(700, 49, .3, .25, 4.5),
    "unsymmetric": unsymmetric_pattern,
    "diagonal": diagonal,
    "hub": hub,
    "wide": wide,
    "long_row": long_row,
    "many_values": many_values,
    "constant_stencil": constant_stencil,
    "upwind": lambda: air_cases.upwind_constant(7, 30),
}
# settings a case is set up with besides relax types 40 / 41 (down / up)
SETTINGS = {"upwind": dict(restriction=1, interp_type=100), "mixed700": dict(strong_threshold=0.25),
            "unsymmetric": dict(strong_threshold=0.25), "hub": dict(strong_threshold=0.25),
            "wide": dict(strong_threshold=0.25), "long_row": dict(strong_threshold=0.25),
            "many_values": dict(strong_threshold=0.25)}


def case(name):
    return CASES[name]()


def settings(name):
    return dict(SETTINGS.get(name, {}))
