"""Operators of the multicolour-ordering tests (tests/test_ilu_color_spec.py, tests/test_gpu_ilu_color.py), each
built once, with its reference ordering (tests/ilu_color_ref.py) computed once and shared.

lap7_16, lap27_10   the 7-point 16^3 and the 27-point 10^3 Laplacian
one                 a 1 x 1 matrix
diagonal            no off-diagonal entry: one colour, one round
path                a tridiagonal matrix (a path graph), 257 rows
dense70             one dense 70 x 70 diagonal block beside 131 sparse rows: 70 colours, the second window of 64
upwind              first-order upwind convection on a 17 x 13 grid: a lower-triangular pattern, every a_ij without a_ji
ragged              601 rows of 1 ... 12 random off-diagonal entries and one row of 300: longer than any lane group
convdiff            upwind convection-diffusion on 9 x 8 x 7 with a velocity that changes sign in space and a downwind
                    correction: unsymmetric values, off-diagonal entries of both signs
Every matrix is strictly diagonally dominant by rows, so ILU(k) exists in any symmetric permutation."""
import numpy as np
import scipy.sparse as sp

from tests import ilu_color_ref as ref
from tests import itilu_ref

NAMES = ("lap7_16", "lap27_10", "one", "diagonal", "path", "dense70", "upwind", "ragged", "convdiff")


def _dominant(M, extra=1.0):
    """M's off-diagonal part with a diagonal of the absolute row sum + extra"""
    M = sp.csr_matrix(M).copy()
    M.setdiag(0.0)
    M.eliminate_zeros()
    d = np.abs(M).sum(axis=1).A1 + extra
    M = (M + sp.diags(d)).tocsr()
    M.sort_indices()
    return M


def _dense70():
    n, m = 201, 70
    rng = np.random.default_rng(70)
    M = sp.lil_matrix((n, n))
    M[:m, :m] = rng.uniform(-1.0, -0.1, size=(m, m))
    for i in range(m, n):  # a chain behind the block, hooked to it at both ends
        M[i, i - 1] = -1.0
        M[i - 1, i] = -0.5
    M[n - 1, 3] = -0.25
    return _dominant(M)


def _upwind():
    nx, ny = 17, 13
    n = nx * ny
    M = sp.lil_matrix((n, n))
    for y in range(ny):
        for x in range(nx):
            i = y * nx + x
            if x > 0:
                M[i, i - 1] = -1.0
            if y > 0:
                M[i, i - nx] = -0.5
    return _dominant(M)


def _ragged():
    n = 601
    rng = np.random.default_rng(601)
    rows, cols = [], []
    for i in range(n):
        k = 300 if i == 417 else int(rng.integers(1, 13))
        c = rng.choice(n, size=k, replace=False)
        rows += [i] * k
        cols += c.tolist()
    M = sp.csr_matrix((rng.uniform(-1.0, 1.0, size=len(rows)), (rows, cols)), shape=(n, n))
    return _dominant(M)


def _convdiff():
    nx, ny, nz = 9, 8, 7
    n = nx * ny * nz
    eps = 0.1
    M = sp.lil_matrix((n, n))
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                i = (z * ny + y) * nx + x
                v = (np.sin(0.9 * x + 0.4 * y), np.cos(0.7 * y - 0.3 * z), np.sin(0.5 * z + 1.1 * x))
                for d, (c, m, stride) in enumerate(((x, nx, 1), (y, ny, nx), (z, nz, nx * ny))):
                    for side in (-1, 1):
                        if not 0 <= c + side < m:
                            continue
                        upwind = (v[d] > 0) == (side < 0)
                        # diffusion, the upwind difference of v d/dx, and a quarter of it back on the downwind side
                        M[i, i + side * stride] = -eps - abs(v[d]) if upwind else -eps + 0.25 * abs(v[d])
    return _dominant(M)


_BUILD = {
    "lap7_16": lambda: itilu_ref.laplace(16, 7),
    "lap27_10": lambda: itilu_ref.laplace(10, 27),
    "one": lambda: sp.csr_matrix(np.array([[2.0]])),
    "diagonal": lambda: sp.diags(np.arange(1.0, 51.0)).tocsr(),
    "path": lambda: sp.diags([-1.0, 2.5, -1.0], [-1, 0, 1], shape=(257, 257)).tocsr(),
    "dense70": _dense70,
    "upwind": _upwind,
    "ragged": _ragged,
    "convdiff": _convdiff,
}
_MATS, _ORD = {}, {}


def matrix(name):
    if name not in _MATS:
        M = sp.csr_matrix(_BUILD[name]()).astype(np.float64)
        M.sort_indices()
        _MATS[name] = M
    return _MATS[name]


def ordering(name):
    """the reference ordering of matrix(name), computed once"""
    if name not in _ORD:
        _ORD[name] = ref.Ordering(matrix(name))
    return _ORD[name]
