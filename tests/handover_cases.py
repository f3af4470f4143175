"""Operators and shared checks of the C-row hand-over tests: tests/test_handover_cases_spec.py
pins on the CPU what each operator is for (C rows, flagged rows, distinct values), and
tests/test_gpu_c_row_handover.py / tests/test_gpu_c_row_handover_paths.py run them through the library.  The
generators need scipy only; the helpers below them take the binding as an argument."""
import numpy as np
import scipy.sparse as sp


def _T(n):
    return sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n))


def _sorted(M, keep_zeros=False):
    M = M.tocsr()
    if not keep_zeros:
        M.eliminate_zeros()  # (scipy's kron stores dense blocks for a small second factor)
    M.sort_indices()
    return M


def lap7(n):
    """The 7-point Dirichlet Laplacian on n^3 points with build_laplace_system's values: 6 and -1."""
    T, I = _T(n), sp.identity(n)
    return _sorted(sp.kron(sp.kron(I, I), T) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(T, I), I))


def lap27(n):
    """The 27-point one: 26 on the diagonal, -1 to each of the up to 26 neighbours."""
    E = sp.diags([1.0, 1.0, 1.0], [-1, 0, 1], shape=(n, n))
    return _sorted(27.0 * sp.identity(n ** 3) - sp.kron(sp.kron(E, E), E))


def aniso(n, k, zc=0.5):
    """7-point operator on n^3 points whose z coupling is zc from plane k on (symmetrised across the step): weak
    there at the app's strong threshold, so C points couple.  k = n // 2: the half-anisotropic operator."""
    T, I = _T(n), sp.identity(n)
    d = np.ones(n)
    d[k:] = zc
    Tz = sp.diags(d) @ T
    Tz = (Tz + Tz.T) * 0.5
    return _sorted(sp.kron(sp.kron(I, I), T) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(Tz, I), I))


def half_anisotropic(n=16, zc=0.5):
    return aniso(n, n // 2, zc)


def scaled(M, seed=3, amp=0.2, sym=True):
    """diag(d1) M diag(d2), d = 1 + amp * (2 u - 1) with u uniform from default_rng(seed); sym: d2 = d1, else d2 is the
    generator's second draw.  Every entry gets a value of its own (level 0 is stored as fp64), and a ratio of
    (1 - amp) / (1 + amp) = 2 / 3 > 0.57 keeps every connection of a Laplacian strong."""
    n = M.shape[0]
    rng = np.random.default_rng(seed)
    d1 = 1.0 + amp * (2.0 * rng.random(n) - 1.0)
    d2 = d1 if sym else 1.0 + amp * (2.0 * rng.random(n) - 1.0)
    return _sorted(sp.diags(d1) @ M @ sp.diags(d2))


def with_explicit_zeros(M, pairs):
    """M with a stored 0.0 at (i, j) and (j, i) for every pair"""
    coo = M.tocoo()
    pi = np.array([p[0] for p in pairs], dtype=np.int64)
    pj = np.array([p[1] for p in pairs], dtype=np.int64)
    rows = np.concatenate([coo.row, pi, pj])
    cols = np.concatenate([coo.col, pj, pi])
    vals = np.concatenate([coo.data, np.zeros(2 * len(pairs))])
    return _sorted(sp.coo_matrix((vals, (rows, cols)), shape=M.shape), keep_zeros=True)


# name -> (builder, n, nc, flagged C rows, more than 256 distinct values) at the app defaults (PMIS, strong threshold
# 0.57), from the oracle's C/F split; tests/test_handover_cases_spec.py asserts every column
CASES = {
    "lap7_9": (lambda: lap7(9), 729, 255, 0, False),
    "lap7_12": (lambda: lap7(12), 1728, 588, 0, False),
    "lap7_12_scaled_sym": (lambda: scaled(lap7(12)), 1728, 588, 0, True),
    "lap7_12_scaled_nonsym": (lambda: scaled(lap7(12), sym=False), 1728, 588, 0, True),
    "lap7_19": (lambda: lap7(19), 6859, 2272, 0, False),
    "lap7_19_scaled_sym": (lambda: scaled(lap7(19)), 6859, 2272, 0, True),
    "lap7_30": (lambda: lap7(30), 27000, 8684, 0, False),
    "lap27_12": (lambda: lap27(12), 1728, 155, 0, False),
    "aniso16_8": (lambda: aniso(16, 8), 4096, 1471, 455, False),
    "aniso16_8_scaled_nonsym": (lambda: scaled(aniso(16, 8), sym=False), 4096, 1438, 359, True),
    "aniso16_4": (lambda: aniso(16, 4), 4096, 1560, 734, False),
    # the smallest sizes with the 65 536 stored entries below which no operator gets a value dictionary (71 632)
    "lap7_22": (lambda: lap7(22), 10648, 3497, 0, False),
    "aniso22_11": (lambda: aniso(22, 11), 10648, 3819, 1163, False),
}
DICTIONARY_MIN_NNZ = 1 << 16  # k::build_value_dictionary
_BUILT = {}


def case(name):
    """the operator of a row of CASES, built once; treat it as read-only"""
    if name not in _BUILT:
        _BUILT[name] = CASES[name][0]()
    return _BUILT[name]


def flagged_rows(M, cf):
    """(nc, flagged): the C rows of a C-first ordered operator with an off-diagonal C column"""
    n = M.shape[0]
    nc = int((np.asarray(cf) == 1).sum())
    rows = np.repeat(np.arange(n), np.diff(M.indptr))
    coupled = (rows < nc) & (M.indices < nc) & (M.indices != rows)
    flagged = np.zeros(n, dtype=bool)
    flagged[rows[coupled]] = True
    return nc, flagged


# ---------------------------------------------------------------------------------------------- library side
def ij_matrix(mi, M):
    N = M.shape[0]
    A = mi.IJMatrix(0, N - 1)
    coo = M.tocoo()
    A.set_values_coo(coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data.astype(np.float64))
    A.assemble()
    return A


def update_values(A, M):
    """an update round of the assembled IJ matrix: every stored entry takes M's value (same pattern)"""
    coo = M.tocoo()
    A.initialize()
    A.set_values_coo(coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data.astype(np.float64))
    A.assemble()


def level0(amg):
    ia, ja, a, shape = amg.level_csr(0, 0)
    return sp.csr_matrix((a, ja, ia), shape=shape), np.asarray(amg.level_cf(0))


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def rowwise_bound(M, z):
    """2 (L + 2) 2^-53 (|M| |z|)_i, L the longest row of M: two fp64 summations of the same at most L products of a
    row, in any two orders, fused or not, each stay within (L + 2) u of the exact sum relative to the sum of the
    magnitudes (L - 1 additions and one rounding per product, first order in u = 2^-53 with one unit to spare for the
    higher orders), so they differ by at most twice that.  Derived, not measured."""
    L = int(np.diff(M.indptr).max())
    return 2.0 * (L + 2) * 2.0 ** -53 * (abs(M) @ np.abs(z))


def check_census(amg, M, cf):
    nc, flagged = flagged_rows(M, cf)
    cen = amg.c_row_handover_census(0)
    assert np.all(cf[:nc] == 1)
    assert cen["flagged_c_rows"] == int(flagged.sum()), (cen, int(flagged.sum()))
    assert cen["listed"] + cen["handed"] == cen["tiles"], cen
    assert 0 <= cen["w_upto"] <= nc
    return cen, nc, flagged


def check_reduced(mi, amg, f, raised=True, label=""):
    """One cycle and the mat-vec after it in mode 0 and in mode 2 on the same f (module docstring of
    tests/test_gpu_c_row_handover_paths.py); leaves mode 2 set.  Returns dict(z, w, w_full, M, cf, census, nc, flagged)."""
    M, cf = level0(amg)
    cen, nc, flagged = check_census(amg, M, cf)
    mi.set_c_row_handover(0)
    z0, w0, w0_full, raised0 = amg.cycle_then_matvec(f)
    assert np.isfinite(z0).all() and np.isfinite(w0_full).all()
    ref = M @ z0
    bound = rowwise_bound(M, z0)
    e_full = np.abs(w0_full - ref)
    print(f"{label}: n {M.shape[0]}, nc {nc} (nc % 8 = {nc % 8}), census {cen}")
    print(f"  full path: max (|w_full - M z| / bound) {(e_full / np.maximum(bound, 1e-300)).max():.3f}")
    assert np.all(e_full <= bound), "the full mat-vec against M z"
    assert not raised0 and same_bits(w0, w0_full)
    mi.set_c_row_handover(2)
    z, w, w_full, got_raised = amg.cycle_then_matvec(f)
    assert got_raised == raised, (got_raised, cen)
    assert same_bits(z, z0), "the extra store changed the cycle"
    assert same_bits(w_full, w0_full)
    assert np.isfinite(w).all(), np.flatnonzero(~np.isfinite(w))[:8]
    e_ref, e_two = np.abs(w - ref), np.abs(w - w_full)
    print(f"  reduced path: max (|w - M z| / bound) {(e_ref / np.maximum(bound, 1e-300)).max():.3f}, "
          f"max (|w - w_full| / bound) {(e_two / np.maximum(bound, 1e-300)).max():.3f}")
    assert np.all(e_ref <= bound), ("the reduced mat-vec against M z, rows", np.flatnonzero(e_ref > bound)[:8])
    assert np.all(e_two <= bound), ("the reduced mat-vec against the full one, rows", np.flatnonzero(e_two > bound)[:8])
    if not raised:
        assert same_bits(w, w_full)
    return dict(z=z, w=w, w_full=w_full, M=M, cf=cf, census=cen, nc=nc, flagged=flagged)
