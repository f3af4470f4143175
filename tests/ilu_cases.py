"""Seeded irregular matrices for the direct (level-scheduled) ILU(k) path and their references (tests/ilu_ref.py),
shared by tests/test_ilu_spec.py and tests/test_gpu_ilu_irregular.py.  Every case is the smallest shape that still runs
the kernel path it is named for; a reference is computed once per process and never changed."""
import numpy as np
import scipy.sparse as sp

from tests import ilu_ref


def _csr(n, entries):
    """entries: {(i, j): value}, no duplicates; columns ascend in the result"""
    keys = sorted(entries)
    M = sp.csr_matrix(([entries[k] for k in keys], ([k[0] for k in keys], [k[1] for k in keys])), shape=(n, n))
    M.sort_indices()
    assert M.nnz == len(keys)
    return M


def _value(rng):
    return float(rng.choice((-1.0, 1.0)) * rng.uniform(0.1, 1.0))


def _dominant(n, ent, rng, factor=1.5, signs=True):
    """set every diagonal to +-(factor * sum|off-diagonal| + 1)"""
    s = np.zeros(n)
    for (i, j), v in ent.items():
        if i != j:
            s[i] += abs(v)
    for i in range(n):
        sg = float(rng.choice((-1.0, 1.0))) if signs else 1.0
        ent[(i, i)] = sg * (factor * s[i] + 1.0)


def ragged(n=600, seed=11):
    """Nonsymmetric, strictly diagonally dominant, mixed signs (the diagonal too): rows of 1 ... 30 entries inside a
    band of +-25, some holding only their diagonal, plus row 310 and column 205 with about 300 entries each."""
    rng = np.random.default_rng(seed)
    R, C = 310, 205
    length = rng.integers(1, 31, size=n)
    length[[0, 17, 333, n - 1]] = 1
    col_rows = set(rng.choice(np.setdiff1d(np.nonzero(length > 1)[0], [C]), size=299, replace=False).tolist())
    ent = {}
    for i in range(n):
        cols = {i}
        if i in col_rows:
            cols.add(C)
        if i == R:
            cols.update(rng.choice(np.setdiff1d(np.arange(n), [R]), size=299, replace=False).tolist())
        else:
            cand = np.setdiff1d(np.arange(max(0, i - 25), min(n, i + 26)), list(cols))
            need = int(length[i]) - len(cols)
            if need > 0:
                cols.update(rng.choice(cand, size=need, replace=False).tolist())
        for j in cols:
            ent[(i, int(j))] = _value(rng)
    _dominant(n, ent, rng)
    return _csr(n, ent)


def chain(n=300, seed=12):
    """Full subdiagonal (one row per lower level set) and 0 ... 5 random entries right of the diagonal in every row."""
    rng = np.random.default_rng(seed)
    ent = {}
    for i in range(n):
        ent[(i, i)] = 0.0
        if i:
            ent[(i, i - 1)] = _value(rng)
        m = min(int(rng.integers(0, 6)), n - 1 - i)
        if m:
            for j in rng.choice(np.arange(i + 1, n), size=m, replace=False):
                ent[(i, int(j))] = _value(rng)
    _dominant(n, ent, rng)
    return _csr(n, ent)


def wide(n=2048 + 5, seed=13):
    """Independent full 2x2 and 3x3 blocks: two or three level sets, the first of more than 256 rows."""
    rng = np.random.default_rng(seed)
    ent, at = {}, 0
    while at < n:
        left = n - at
        m = left if left <= 3 else (2 if left == 4 else int(rng.integers(2, 4)))
        for i in range(at, at + m):
            for j in range(at, at + m):
                ent[(i, j)] = _value(rng)
        at += m
    _dominant(n, ent, rng)
    return _csr(n, ent)


def arrow(n=400, seed=14):
    """Dense last row and last column on a sparse band: the last row depends on every other row."""
    rng = np.random.default_rng(seed)
    ent = {}
    for i in range(n):
        ent[(i, i)] = 0.0
        ent[(i, n - 1)] = _value(rng)
        ent[(n - 1, i)] = _value(rng)
        cand = np.setdiff1d(np.arange(max(0, i - 10), min(n - 1, i + 11)), [i])
        for j in rng.choice(cand, size=min(3, len(cand)), replace=False):
            ent[(i, int(j))] = _value(rng)
    _dominant(n, ent, rng)
    return _csr(n, ent)


ONESIDED_SEED, ONESIDED_DIAG = 15, 0.8


def onesided(n=500, seed=ONESIDED_SEED, diag=ONESIDED_DIAG):
    """Structurally unsymmetric (a_ij stored only where a_ji is not) and not diagonally dominant: the diagonal is
    `diag` times the row's off-diagonal sum.  Seed and scaling are chosen so that no pivot of ILU(0 ... 2) comes near
    zero (tests/test_ilu_spec.py asserts min|u_kk| >= 1e-3 max|a_ij| in the longdouble reference)."""
    rng = np.random.default_rng(seed)
    ent = {}
    for i in range(n):
        cand = np.setdiff1d(np.arange(max(0, i - 20), min(n, i + 21)), [i])
        for j in rng.choice(cand, size=6, replace=False):
            if (int(j), i) not in ent:
                ent[(i, int(j))] = _value(rng)
    s = np.zeros(n)
    for (i, j), v in ent.items():
        s[i] += abs(v)
    for i in range(n):
        ent[(i, i)] = diag * s[i] + 0.05
    return _csr(n, ent)


def tiny1():
    return sp.csr_matrix(np.array([[-2.5]]))


def tiny2():
    return sp.csr_matrix(np.array([[4.0, -1.0], [2.0, 3.0]]))


def tiny3():
    """3x3 with an empty strict lower part"""
    return _csr(3, {(0, 0): 2.0, (0, 2): -1.0, (1, 1): -3.0, (1, 2): 0.5, (2, 2): 4.0})


def refused(kind):
    """(matrix, local row the setup must name): 6x6 block-diagonal matrices without an ILU factorisation.
    'missing': row 2 stores no diagonal; 'stored_zero': a_44 = 0 is stored and no elimination changes it;
    'eliminated': the block [[1,1],[1,1]] in rows 2, 3 gives u_33 = 1 - 1 * 1; 'good': that block with a_33 = 4."""
    if kind == "missing":
        rows, cols = [0, 1, 2, 3, 3, 4, 4, 5, 5], [0, 1, 3, 2, 3, 4, 5, 4, 5]
        vals, bad = [4.0, 4.0, 1.0, 1.0, 4.0, 4.0, 1.0, 1.0, 4.0], 2
    elif kind == "stored_zero":
        rows, cols = [0, 1, 2, 2, 3, 3, 4, 4, 5, 5], [0, 1, 2, 3, 2, 3, 4, 5, 4, 5]
        vals, bad = [4.0, 4.0, 4.0, 1.0, 1.0, 4.0, 0.0, 1.0, 1.0, 4.0], 4
    else:
        rows, cols = [0, 1, 2, 2, 3, 3, 4, 5], [0, 1, 2, 3, 2, 3, 4, 5]
        vals, bad = [4.0, 4.0, 1.0, 1.0, 1.0, 1.0 if kind == "eliminated" else 4.0, 4.0, 4.0], 3
    return sp.csr_matrix((vals, (rows, cols)), shape=(6, 6)), (bad if kind != "good" else None)


BUILDERS = dict(ragged=ragged, chain=chain, wide=wide, arrow=arrow, onesided=onesided, tiny1=tiny1, tiny2=tiny2,
                tiny3=tiny3)
FILLS = dict(ragged=(0, 1, 2), chain=(0, 1, 2), arrow=(0, 1, 2), onesided=(0, 1, 2), wide=(0,), tiny1=(0,),
             tiny2=(0,), tiny3=(0,))
ALL = [(name, fill) for name in BUILDERS for fill in FILLS[name]]
IDS = [f"{name}-fill{fill}" for name, fill in ALL]
JACOBI_ITS = ((0, 0), (1, 0), (0, 1), (2, 3), (3, 2))

_MATRICES, _REFS = {}, {}


def matrix(name):
    if name not in _MATRICES:
        _MATRICES[name] = BUILDERS[name]()
    return _MATRICES[name]


class Reference:
    """Pattern, longdouble and float64 factors of one case at one fill, a seeded right-hand side, and the exact and
    Jacobi applications to it in both precisions (computed on first use)."""

    def __init__(self, name, fill):
        self.A = matrix(name)
        self.n = self.A.shape[0]
        self.ia, self.ja = ilu_ref.symbolic(self.A, fill)
        self.ld = ilu_ref.Factors(self.A, fill, ilu_ref.LD, pattern=(self.ia, self.ja))
        self.f64 = ilu_ref.Factors(self.A, fill, np.float64, pattern=(self.ia, self.ja))
        self.levels = ilu_ref.level_sets(self.ia, self.ja)
        self.rhs = np.random.default_rng(1000 + 10 * sorted(BUILDERS).index(name) + fill).standard_normal(self.n)
        self._applied = {}

    def applied(self, its=None):
        """(longdouble, float64) application to rhs: exact for its None, else Jacobi with its = (lower, upper)"""
        if its not in self._applied:
            self._applied[its] = tuple(F.apply_exact(self.rhs) if its is None else F.apply_jacobi(self.rhs, *its)
                                       for F in (self.ld, self.f64))
        return self._applied[its]

    def nilpotency_its(self):
        return (self.levels[0] - 1, self.levels[1] - 1)


def multivector_rhs():
    """Three right-hand sides on `ragged` that a Richardson solve with ILU(0) finishes after different numbers of
    steps when each is solved alone (tests/test_ilu_spec.py asserts it): b = A x for x = 1, a unit vector, noise."""
    A = matrix("ragged")
    n = A.shape[0]
    e = np.zeros(n)
    e[0] = 1.0
    return np.stack([A @ np.ones(n), A @ e, 50.0 * np.random.default_rng(77).standard_normal(n)])


def reference(name, fill):
    if (name, fill) not in _REFS:
        _REFS[(name, fill)] = Reference(name, fill)
    return _REFS[(name, fill)]
