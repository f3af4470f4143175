"""CPU: the FSAI entry points are declared and exported, and the numpy restatement the GPU tests compare against
(tests/fsai_ref.py) satisfies the identities of its specification ("FSAI")."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from tests import fsai_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FSAI_SYMBOLS = (
    ["HYPRE_BoomerAMGSetFSAI" + s for s in ("AlgoType", "LocalSolveType", "NumLevels", "Threshold", "EigMaxIters",
                                            "MaxSteps", "MaxStepSize", "MaxNnzRow", "KapTolerance")]
    + ["HYPRE_FSAI" + s for s in ("Create", "Destroy", "Setup", "Solve")]
    + ["HYPRE_FSAISet" + s for s in ("AlgoType", "NumLevels", "Threshold", "EigMaxIters", "Omega", "MaxIterations",
                                     "Tolerance", "ZeroGuess", "PrintLevel")]
    + ["HYPRE_MI_BoomerAMGGetLevelFSAISize", "HYPRE_MI_BoomerAMGGetLevelFSAI", "HYPRE_MI_BoomerAMGSmoothLevel"])


def test_fsai_symbols_declared_and_exported(mi_lib):
    text = ""
    for h in ("HYPRE_parcsr_ls.h", "HYPRE_mi_ext.h"):
        text += re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
    lib = mi_lib.lib()
    for name in FSAI_SYMBOLS:
        assert re.search(r"HYPRE_Int\s+" + name + r"\s*\(", text), name
        assert hasattr(lib, name), name


def _laplace2d(n):
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n))
    I = sp.identity(n)
    return (sp.kron(I, T) + sp.kron(T, I)).tocsr()


def _random_spd(n, seed):
    rng = np.random.default_rng(seed)
    R = sp.random(n, n, density=0.08, random_state=rng, data_rvs=lambda k: -rng.random(k))
    R = R + R.T
    R.setdiag(0.0)
    d = -np.asarray(R.sum(axis=1)).ravel() + 0.5 + rng.random(n)
    return (R + sp.diags(d)).tocsr()


@pytest.mark.parametrize("case,theta,k", [("lap", 0.0, 1), ("lap", 0.01, 2), ("rand", 0.3, 1), ("rand", 0.0, 3)])
def test_restatement_satisfies_local_identities(case, theta, k):
    """For SPD B: diag(G B G^T) = 1 and (G B)_ij = 0 for every j in P_i other than i; G lower triangular."""
    B = _laplace2d(6) if case == "lap" else _random_spd(40, 3)
    P = fsai_ref.pattern(B, theta, k)
    G = fsai_ref.factor(B, theta, k, pat=P)
    assert sp.triu(G, 1).nnz == 0
    GB = (G @ B).toarray()
    assert np.allclose(np.diag((G @ B @ G.T).toarray()), 1.0, rtol=1e-13)
    for i, p in enumerate(P):
        off = [j for j in p if j != i]
        assert np.abs(GB[i, off]).max(initial=0.0) < 1e-13 * np.abs(GB[i]).max()
    # k = 1, theta = 0: the lower triangle of B
    if theta == 0.0 and k == 1:
        L = sp.tril(B).tocsr()
        assert all(np.array_equal(P[i], L.indices[L.indptr[i]:L.indptr[i + 1]]) for i in range(B.shape[0]))


def test_full_lower_pattern_gives_inverse():
    """With the whole lower triangle as pattern, G^T G = B^-1 (G is the inverse Cholesky factor)."""
    B = _random_spd(30, 5)
    n = B.shape[0]
    full = [np.arange(i + 1) for i in range(n)]
    G = fsai_ref.factor(B, pat=full).toarray()
    assert np.allclose(G.T @ G, np.linalg.inv(B.toarray()), rtol=1e-10, atol=1e-12)


def test_pivot_tie_takes_lowest_row_and_bad_rows_are_reported():
    # equal |values| in the first column: the lowest row is the pivot (result independent of ties for exact data)
    M = np.array([[2.0, -2.0, 0.0], [-2.0, 5.0, 1.0], [0.0, 1.0, 3.0]])
    y = fsai_ref.local_solve(M)
    assert np.allclose(M.T @ y, [0.0, 0.0, 1.0])
    with pytest.raises(np.linalg.LinAlgError):
        fsai_ref.local_solve(np.zeros((2, 2)))
    B = sp.csr_matrix(np.array([[1.0, 2.0], [2.0, 1.0]]))  # indefinite: y_last < 0 in row 1
    with pytest.raises(ValueError, match="row 1"):
        fsai_ref.factor(B, theta=0.0)
