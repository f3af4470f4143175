"""Inputs of the kernel tests of the matrix-matrix extended interpolation (tests/test_gpu_mm_interp.py): operators,
strength patterns and markers handed straight to HYPRE_MI_MMInterpOp, and a census of the cases they hold.  Everything
is generated from seeds; the strength pattern and the marker of the crafted operator are chosen freely (the routine takes
them as inputs), so that every branch of the left-operand kernel meets a row."""
import numpy as np
import scipy.sparse as sp

from tests import mm_interp_ref as ref

LANES = (1, 2, 4, 8, 16, 32, 64)


def _csr(rows, n):
    indptr, indices, data = [0], [], []
    for r in rows:
        for c in sorted(r):
            indices.append(c)
            data.append(r[c])
        indptr.append(len(indices))
    return sp.csr_matrix((np.array(data, dtype=float), np.array(indices, dtype=np.int64), np.array(indptr)), shape=(n, n))


def _pattern(sets, n):
    indptr = np.cumsum([0] + [len(s) for s in sets])
    indices = np.array([c for s in sets for c in sorted(s)], dtype=np.int64)
    return sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(n, n))


def greedy_marker(strong):
    """a maximal independent set of the symmetrised strength graph in row order: C = +1, its neighbours F = -1, rows
    without a strong neighbour special F = -3"""
    n = len(strong)
    nb = [set(int(j) for j in s) for s in strong]
    for i, s in enumerate(strong):
        for j in s:
            nb[int(j)].add(i)
    m = np.zeros(n, dtype=np.int64)
    for i in range(n):
        if len(strong[i]) == 0:
            m[i] = -3
    for i in range(n):
        if m[i] == 0:
            m[i] = 1
            for j in nb[i]:
                if m[j] == 0:
                    m[j] = -1
    return m


def ragged(n=2000, seed=5):
    """A ragged M-matrix: rows of 1 to ~30 entries and one of ~300; half of the off-diagonal entries have a stored
    transposed partner, the others have none.  Strength by the library's rule at theta = 0.25, marker greedy."""
    rng = np.random.default_rng(seed)
    rows = [dict() for _ in range(n)]
    for i in range(n):
        k = 300 if i == 777 else int(rng.integers(0, 20))
        for j in rng.choice(n, size=k, replace=False):
            j = int(j)
            if j == i:
                continue
            rows[i][j] = -float(rng.uniform(0.1, 1.0))
            if rng.random() < 0.5 and len(rows[j]) < 29:
                rows[j].setdefault(i, -float(rng.uniform(0.1, 1.0)))
    for i in range(n):
        rows[i][i] = -sum(rows[i].values()) + float(rng.uniform(0.1, 1.0))
    A = _csr(rows, n)
    strong = ref.strength_rows(A, 0.25)
    return A, strong, _pattern(strong, n), greedy_marker(strong)


def crafted(seed=11):
    """200 rows.  Rows 0 ... 19: F rows with exactly G - 1, G and G + 1 strong neighbours (and the diagonal) for every
    G in LANES.  Rows 170 ... 179 are C points.  Named pairs (F row i, strong F neighbour k): (100, 150) a_ki stored
    first in row k, (190, 120) stored last, (101, 151) absent; (102, 152) beta_k = 0; (104, 154) a_ki = -beta_k; row 103
    has only C neighbours, row 105 no strong neighbour.  Everything else is random."""
    n = 200
    rng = np.random.default_rng(seed)
    rows = [dict() for _ in range(n)]
    S = [set() for _ in range(n)]
    m = np.zeros(n, dtype=np.int64)
    others = np.arange(20, n)
    i = 0
    for G in LANES:
        for c in (G - 1, G, G + 1):
            if c < 1:
                continue
            for j in rng.choice(others, size=c, replace=False):
                rows[i][int(j)] = -float(rng.uniform(0.5, 2.0))
                S[i].add(int(j))
            m[i] = -1
            i += 1
    assert i == 20
    for i in range(20, n):
        for j in rng.choice(n, size=int(rng.integers(2, 7)), replace=False):
            j = int(j)
            if j == i:
                continue
            rows[i][j] = -float(rng.uniform(0.2, 2.0))
            if rng.random() < 0.6:
                S[i].add(j)
        m[i] = rng.choice([1, 1, -1, -1, -1, -3], p=None)
    m[170:180] = 1
    special = {100, 150, 190, 120, 101, 151, 102, 152, 103, 104, 154, 105}
    for r in special:
        rows[r], S[r] = dict(), set()
        m[r] = -1
    # scrub what the random rows stored towards the named rows' partners where the case depends on it
    for r in range(n):
        if r not in special:
            for c in special:
                if c in rows[r] and r >= 20:
                    del rows[r][c]
                    S[r].discard(c)

    def strong_c(k, cols_vals):
        for c, v in cols_vals:
            rows[k][c] = v
            S[k].add(c)
    # a_ki stored first: row 150 stores column 100 and nothing before it
    rows[100].update({150: -1.25, 171: -0.75}), S[100].update({150, 171})
    strong_c(150, [(172, -1.0), (175, -0.5)])
    rows[150][100] = -0.625
    # stored last: row 120 stores column 190 and nothing after it
    rows[190].update({120: -1.5, 173: -0.5}), S[190].update({120, 173})
    strong_c(120, [(170, -1.0), (174, -0.25)])
    rows[120][190] = -0.375
    # absent: row 151 does not store column 101
    rows[101].update({151: -1.0, 176: -0.5}), S[101].update({151, 176})
    strong_c(151, [(177, -1.0), (178, -2.0)])
    # beta_k = 0: row 152 has no strong C neighbour
    rows[102].update({152: -1.0, 179: -0.5, 30: -0.25}), S[102].update({152, 179})
    rows[152].update({102: -0.5, 171: -0.125})
    # only C neighbours, strong and weak
    rows[103].update({170: -1.0, 175: -0.75, 179: -0.125}), S[103].update({170, 175})
    # delta_ki = 0: beta_154 = -1.5 exactly, a_(154, 104) = +1.5
    rows[104].update({154: -1.0, 172: -0.5}), S[104].update({154, 172})
    strong_c(154, [(173, -1.0), (176, -0.5)])
    rows[154][104] = 1.5
    # no strong neighbour at all (an F point all the same)
    rows[105].update({171: -0.25, 31: -0.125})
    for r in range(n):
        rows[r][r] = 10.0 + float(rng.uniform(0.0, 1.0))
    A = _csr(rows, n)
    strong = [np.array(sorted(s), dtype=int) for s in S]
    return A, strong, _pattern(S, n), m


def census(A, strong, m):
    """which of the kernel's cases the input holds (counts)"""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    row = lambda i: dict(zip(A.indices[A.indptr[i]:A.indptr[i + 1]].tolist(), A.data[A.indptr[i]:A.indptr[i + 1]].tolist()))
    beta = np.zeros(n)
    for k in range(n):
        rk = row(k)
        for l in sorted(rk):
            if l in set(strong[k].tolist()) and m[l] == 1:
                beta[k] += rk[l]
    out = dict(first=0, last=0, absent=0, middle=0, beta_zero=0, delta_zero=0, f_no_strong=0, f_only_c=0)
    for G in LANES:
        out["strong%d" % G] = out["strong%d" % (G + 1)] = 0
    for i in range(n):
        if m[i] != -1:
            continue
        ns = len(strong[i])
        if "strong%d" % ns in out:
            out["strong%d" % ns] += 1
        if ns == 0:
            out["f_no_strong"] += 1
        elif all(m[k] == 1 for k in row(i) if k != i):
            out["f_only_c"] += 1
        for k in strong[i]:
            k = int(k)
            if m[k] == 1:
                continue
            if beta[k] == 0.0:
                out["beta_zero"] += 1
                continue
            cols = sorted(row(k))
            if i not in cols:
                out["absent"] += 1
                continue
            out["first" if cols[0] == i else "last" if cols[-1] == i else "middle"] += 1
            if beta[k] + row(k)[i] == 0.0:
                out["delta_zero"] += 1
    return out
