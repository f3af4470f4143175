"""Seeded test matrices for FSAI with the adaptive pattern (fsai_algo_type 4), shared by the CPU and the GPU tests, and
the cached restatement results on them (tests/fsai_adaptive_ref.py)."""
import functools

import numpy as np
import scipy.sparse as sp

from tests import fsai_adaptive_ref as ref


def lap7(n, weights=(1.0, 1.0, 1.0)):
    """7-point operator on n^3 points, lexicographic; weights (x, y, z) scale the three second differences."""
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n))
    I = sp.identity(n)
    wx, wy, wz = weights
    return (wx * sp.kron(sp.kron(I, I), T) + wy * sp.kron(sp.kron(I, T), I) + wz * sp.kron(sp.kron(T, I), I)).tocsr()


def lap27(n):
    """27-point operator on n^3 points: 26 on the diagonal, -1 to each of the up to 26 neighbours."""
    E = sp.diags([1.0, 1.0, 1.0], [-1, 0, 1], shape=(n, n))
    return (27.0 * sp.identity(n ** 3) - sp.kron(sp.kron(E, E), E)).tocsr()


def ragged(n=1500, seed=12, long_row=60):
    """random nonsymmetric M-matrix: rows of 1 ... ~30 lower entries and a last row with ~long_row of them."""
    rng = np.random.default_rng(seed)
    M = sp.random(n, n, density=24.0 / n, random_state=rng, format="lil")
    for c in rng.choice(n - 1, size=long_row, replace=False):
        M[n - 1, c] = rng.standard_normal()
    M = M.tocsr()
    M.setdiag(0.0)
    M.eliminate_zeros()
    M = -abs(M)
    return (M + sp.diags(np.abs(M).sum(axis=1).A1 * 1.01 + 1e-3)).tocsr()


def tridiagonal(n):
    return sp.diags([-1.0, 2.5, -1.0], [-1, 0, 1], shape=(n, n)).tocsr()


def indefinite_block():
    """y_last <= 0 in row 6: an indefinite 2 x 2 block in rows 5, 6 of a diagonal matrix."""
    M = sp.diags(np.full(10, 4.0)).tolil()
    M[5, 5], M[6, 6], M[5, 6], M[6, 5] = 1.0, 1.0, 2.0, 2.0
    return M.tocsr()


def missing_diagonal():
    """row 3 stores no diagonal entry: its first local system is singular."""
    M = tridiagonal(9).tolil()
    M[3, 3] = 0.0
    M = M.tocsr()
    M.eliminate_zeros()
    return M


# name -> builder; every matrix has sorted rows.  `lap*` are full of exact ties between candidates; `short_rows` has
# rows with fewer candidates than max_step_size; n = 5 is not a multiple of the rows per wave.
CASES = {
    "lap7_8": lambda: lap7(8),
    "lap7_12": lambda: lap7(12),
    "lap27_8": lambda: lap27(8),
    "lap27_10": lambda: lap27(10),
    "aniso_8": lambda: lap7(8, (1.0, 1.0, 100.0)),
    "ragged": lambda: ragged(),
    "ragged_small": lambda: ragged(300, seed=5, long_row=80),
    "diagonal": lambda: sp.diags(np.linspace(1.0, 3.0, 37)).tocsr(),
    "one_row": lambda: sp.csr_matrix(np.array([[2.0]])),
    "five_rows": lambda: tridiagonal(5),
    "short_rows": lambda: tridiagonal(40),
}
FAILING = {"indefinite_block": (indefinite_block, 6, "y_last"), "missing_diagonal": (missing_diagonal, 3, "singular")}
DEFAULTS = (3, 5, 1e-3)


@functools.lru_cache(maxsize=None)
def matrix(name):
    M = (CASES[name] if name in CASES else FAILING[name][0])()
    M = sp.csr_matrix(M, dtype=np.float64)
    M.sort_indices()
    return M


@functools.lru_cache(maxsize=None)
def reference(name, max_steps=3, max_step_size=5, kap_tolerance=1e-3):
    """(G, info) of the restatement; computed once per parameter set and never changed by a test."""
    return ref.factor(matrix(name), max_steps, max_step_size, kap_tolerance)


def as_csr(triple):
    ia, ja, a, shape = triple
    return sp.csr_matrix((a, ja, ia), shape=shape)


def same_G(G, Gr):
    """equal patterns, values within the project's FSAI tolerance (tests/test_gpu_fsai.py): 1e-12 of max |G|"""
    assert np.array_equal(G.indptr, Gr.indptr) and np.array_equal(G.indices, Gr.indices)
    err = np.abs(G.data - Gr.data).max()
    assert err <= 1e-12 * np.abs(Gr.data).max(), err


def same_counts(info, rinfo):
    """the op's info[] against the restatement's counts"""
    assert info["status"] == 0 and info["bad_row"] == -1
    assert info["max_row"] == rinfo["max_row"] and info["max_candidates"] == rinfo["max_candidates"]
    assert info["stop_tolerance"] == rinfo["stops"][ref.STOP_TOL]
    assert info["stop_no_candidate"] == rinfo["stops"][ref.STOP_NO_CANDIDATE]
    assert info["stop_max_steps"] == rinfo["stops"][ref.STOP_MAX_STEPS]
