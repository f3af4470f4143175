"""C-row hand-over beyond the default smoother and the Laplacians: the paths that
tests/test_gpu_c_row_handover.py does not reach.  Operators: tests/handover_cases.py (what each is for is pinned on the
CPU by tests/test_handover_cases_spec.py).

The common check (handover_cases.check_reduced) runs one cycle from a zero guess and the mat-vec after it
(HYPRE_MI_BoomerAMGCycleThenMatvec, which pre-fills w with NaN) on the same f in mode 0 and in mode 2 and asserts
  * mode 0: not raised, w = w_full bit for bit, and w_full within the row-wise bound of scipy's M z (asserted first, so a
    failure names the path);
  * mode 2: raised, the same z bit for bit (the extra store must not change the cycle), w finite on every row, and for
    every row i both |w_i - (M z)_i| and |w_i - w_full_i| <= 2 (L + 2) 2^-53 (|M| |z|)_i with L the longest row of M:
    the worst case of two fp64 summations of the same at most L products in different orders, fused or not -- derived
    (handover_cases.rowwise_bound), not measured;
  * the census: flagged_c_rows is the number of C rows of level_csr / level_cf with an off-diagonal C column, and
    listed + handed = tiles.

  (a) every value format of level 0.  A value dictionary needs at most 256 distinct values and at least 65 536 stored
      entries, so the 12^3 and 16^3 operators are fp64 (kind 0) with the switch on or off, as are the scaled ones
      with a value per entry; the 22^3 operators are the smallest the switch decides (kind 8 on, 0 off).  Both the FP64
      and the DICT instantiation of the tile kernel store wout, and the listed-tile mat-vec streams either format;
  (b) relax types 3 / 4 / 6 / 13 / 14 and mixed down / up types, with weights 1 and (relax 0.8, outer 1.1): wout must be
      S + a_ii u_new with the matrix diagonal, whatever the sweep divides by; two up sweeps, a W-cycle, an aggressive
      first level;
  (c) nc a multiple of 8, nc beyond one super-block of 8192 rows, nc < 256 (nothing handed over, no list), and the 10 %
      threshold of mode 1;
  (d) work vectors poisoned with NaN before the cycle;
  (e) the relax type and the chunk size changed after Setup, and changed back;
  (f) a refresh (setup reuse) on new values: the census is of the pattern and stays, the values are the new ones -- also
      when the refresh leaves the value dictionary, and when the flagged rows are flagged by stored zeros;
  (g) the Krylov loops: restarts, FlexGMRES, COGMRES, kept directions off, a non-zero initial guess, a solve cut by
      max_iterations, two solves on the same objects, the threshold inside a solve, a stale hierarchy.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import handover_cases as hc

pytestmark = pytest.mark.gpu

_A = {}


def matrix(mi, name):
    """the IJ matrix of a case, assembled once per module (value dictionary on); never updated in place"""
    if name not in _A:
        _A[name] = hc.ij_matrix(mi, hc.case(name))
    return _A[name]


@pytest.fixture(autouse=True)
def switches(mi):
    """the process-wide switches the tests touch go back to their defaults"""
    yield
    mi.set_c_row_handover(1)
    mi.set_value_dictionary(True)
    mi.call("HYPRE_MI_SetGSChunk", 8)
    mi.set_gmres_keep_directions(True)


def rhs(n, seed=5):
    return np.random.default_rng(seed).standard_normal(n)


def hierarchy(mi, A, **kw):
    amg = mi.BoomerAMG(print_level=0, **kw)
    amg.setup(A)
    return amg


def assert_both_kinds_of_tile(r):
    """flagged rows exist, handed-over tiles exist, and a listed tile is made of C rows alone: a tile has at most 512
    rows, so the tile of a flagged row that far below nc ends among the C rows"""
    assert r["census"]["flagged_c_rows"] > 0 and r["census"]["handed"] > 0
    assert r["flagged"][:max(r["nc"] - 512, 0)].any()


# ------------------------------------------------------------------------------------------------- (a) fp64 values
# (a value dictionary needs at most 256 distinct values AND at least 65 536 stored entries: the plain 12^3 and 16^3
# 7-point operators are fp64 with the switch on or off; the 22^3 ones are the smallest that the switch decides)
@pytest.mark.parametrize("name,dictionary,kind,both_kinds", [
    ("lap7_12_scaled_sym", True, 0, False),
    ("lap7_12_scaled_nonsym", True, 0, False),
    ("aniso16_8_scaled_nonsym", True, 0, True),
    ("lap7_12", False, 0, False),
    ("lap7_12", True, 0, False),
    ("lap7_22", False, 0, False),
    ("lap7_22", True, 8, False),
    ("aniso22_11", False, 0, True),
    ("aniso22_11", True, 8, True),
], ids=["scaled_sym", "scaled_nonsym", "scaled_aniso", "lap12_dictionary_off", "lap12_too_small_for_a_dictionary",
        "lap22_dictionary_off", "lap22_dictionary", "aniso22_dictionary_off", "aniso22_dictionary"])
def test_fp64_level0(mi, name, dictionary, kind, both_kinds):
    mi.set_value_dictionary(dictionary)
    A = matrix(mi, name) if dictionary else hc.ij_matrix(mi, hc.case(name))
    amg = hierarchy(mi, A)
    assert amg.level_value_storage(0, 0)[0] == kind
    r = hc.check_reduced(mi, amg, rhs(A.iupper + 1), raised=True, label=name)
    assert r["census"]["handed"] > 0 and 0 < r["census"]["w_upto"] <= r["nc"]
    if both_kinds:
        assert_both_kinds_of_tile(r)
    else:
        assert r["census"]["flagged_c_rows"] == 0


# ------------------------------------------------------------------------------------------- (b) smoother settings
@pytest.mark.parametrize("weights", [(1.0, 1.0), (0.8, 1.1)], ids=["w1", "w0.8_1.1"])
@pytest.mark.parametrize("down,up", [(3, 3), (4, 4), (6, 6), (13, 14), (14, 13), (8, 3)])
@pytest.mark.parametrize("name", ["aniso16_8", "aniso16_8_scaled_nonsym", "aniso22_11"])  # fp64, fp64, dictionary
def test_relax_types_and_weights(mi, name, down, up, weights):
    A = matrix(mi, name)
    amg = hierarchy(mi, A, down_relax_type=down, up_relax_type=up, coarse_relax_type=9, relax_weight=weights[0],
                    outer_weight=weights[1])
    r = hc.check_reduced(mi, amg, rhs(A.iupper + 1), raised=True, label=f"{name} {down}/{up} {weights}")
    assert_both_kinds_of_tile(r)


def test_weights_reach_the_smoother(mi):
    """the keys relax_weight / outer_weight are not decoration: the cycle's z moves with them"""
    A = matrix(mi, "aniso16_8")
    f = rhs(A.iupper + 1)
    kw = dict(down_relax_type=3, up_relax_type=3, coarse_relax_type=9)
    z1 = hierarchy(mi, A, relax_weight=1.0, outer_weight=1.0, **kw).cycle_then_matvec(f)[0]
    assert hc.same_bits(z1, hierarchy(mi, A, **kw).cycle_then_matvec(f)[0])
    for rw, ow in ((0.8, 1.0), (1.0, 1.1)):
        z = hierarchy(mi, A, relax_weight=rw, outer_weight=ow, **kw).cycle_then_matvec(f)[0]
        assert np.abs(z - z1).max() > 1e-3 * np.abs(z1).max()


@pytest.mark.parametrize("label,kw", [
    ("two_up_sweeps", dict(num_down_sweeps=1, num_up_sweeps=2, num_coarse_sweeps=1)),
    ("w_cycle", dict(cycle_type=2)),
    ("aggressive_level", dict(agg_num_levels=1)),
], ids=lambda v: v if isinstance(v, str) else None)
@pytest.mark.parametrize("name", ["aniso16_8", "aniso22_11"])
def test_cycle_shapes(mi, name, label, kw):
    """Two up sweeps: only the last pair may hand over.  An aggressive first level leaves the 16^3 operator 340 C rows,
    39 of them flagged and 25 of those among the first 256: no tile is handed over, nothing is raised and w is the full
    mat-vec; the 22^3 operator keeps 844, the first 256 unflagged: one handed-over tile."""
    A = matrix(mi, name)
    amg = hierarchy(mi, A, **kw)
    handed = (name, label) != ("aniso16_8", "aggressive_level")
    r = hc.check_reduced(mi, amg, rhs(A.iupper + 1), raised=handed, label=f"{name} {label}")
    assert (r["census"]["handed"] > 0) == handed and r["census"]["flagged_c_rows"] > 0
    if label == "aggressive_level":
        assert r["nc"] == (340 if name == "aniso16_8" else 844)


# ----------------------------------------------------------------------------------------------------- (c) edges
@pytest.mark.parametrize("name", ["lap7_19", "lap7_19_scaled_sym", "aniso16_4"])
def test_nc_multiple_of_8(mi, name):
    A = matrix(mi, name)
    amg = hierarchy(mi, A)
    r = hc.check_reduced(mi, amg, rhs(A.iupper + 1), raised=True, label=name)
    assert r["nc"] % 8 == 0 and r["nc"] == int((np.asarray(amg.level_cf(0)) == 1).sum())
    assert r["census"]["handed"] > 0


def test_c_rows_beyond_a_super_block(mi):
    A = matrix(mi, "lap7_30")
    amg = hierarchy(mi, A)
    r = hc.check_reduced(mi, amg, rhs(A.iupper + 1), raised=True, label="lap7_30")
    assert r["nc"] > 8192 and r["census"]["w_upto"] > 8192


def test_fewer_c_rows_than_a_tile(mi):
    A = matrix(mi, "lap7_9")
    amg = hierarchy(mi, A)
    r = hc.check_reduced(mi, amg, rhs(A.iupper + 1), raised=False, label="lap7_9")  # mode 2: w = w_full bit for bit
    cen = r["census"]
    assert r["nc"] < 256
    assert cen["handed"] == 0 and cen["listed"] == cen["tiles"] and cen["w_upto"] == 0


@pytest.mark.parametrize("name", ["aniso16_4", "lap27_12"])
def test_threshold_of_mode_1(mi, name):
    A = matrix(mi, name)
    amg = hierarchy(mi, A)
    cen = amg.c_row_handover_census(0)
    print(f"{name}: census {cen}")
    assert 0 < 10 * cen["handed"] < cen["tiles"]
    f = rhs(A.iupper + 1)
    r = hc.check_reduced(mi, amg, f, raised=True, label=name)
    mi.set_c_row_handover(1)
    z, w, w_full, raised = amg.cycle_then_matvec(f)
    assert not raised and hc.same_bits(w, w_full) and hc.same_bits(z, r["z"])


# --------------------------------------------------------------------------------------- (d) poisoned work vectors
@pytest.mark.parametrize("name", ["aniso16_8", "lap7_12_scaled_sym", "aniso22_11"])
def test_poisoned_work_vectors(mi, name):
    A = matrix(mi, name)
    amg = hierarchy(mi, A)
    f = rhs(A.iupper + 1)
    mi.set_c_row_handover(2)
    z, w, w_full, raised = amg.cycle_then_matvec(f)
    assert raised and np.isfinite(w).all()
    mi.call("HYPRE_MI_BoomerAMGPoisonWorkVectors", amg.h)
    zp, wp, wp_full, raised_p = amg.cycle_then_matvec(f)
    assert raised_p
    assert hc.same_bits(zp, z) and hc.same_bits(wp, w) and hc.same_bits(wp_full, w_full)


# ------------------------------------------------------------------------------- (e) settings changed after Setup
def test_settings_changed_after_setup(mi):
    A = matrix(mi, "aniso16_8")
    amg = hierarchy(mi, A)
    f = rhs(A.iupper + 1)
    M, cf = hc.level0(amg)
    mi.set_c_row_handover(2)
    assert amg.cycle_then_matvec(f)[3]
    mi.call("HYPRE_BoomerAMGSetRelaxType", amg.h, 16)
    z, w, w_full, raised = amg.cycle_then_matvec(f)
    assert not raised and np.isfinite(w).all() and hc.same_bits(w, w_full)
    mi.call("HYPRE_BoomerAMGSetRelaxType", amg.h, 8)
    assert amg.cycle_then_matvec(f)[3]
    mi.call("HYPRE_MI_SetGSChunk", 4)
    z, w, w_full, raised = amg.cycle_then_matvec(f)
    assert not raised and np.isfinite(w).all()
    assert np.all(np.abs(w - M @ z) <= hc.rowwise_bound(M, z))
    mi.call("HYPRE_MI_SetGSChunk", 8)
    hc.check_reduced(mi, amg, f, raised=True, label="chunk back to 8")


# --------------------------------------------------------------------------------------------------- (f) setup reuse
def _refreshed(mi, M1, M2, kind1, kind2, label):
    """Setup on M1 with setup reuse on, an update round to M2's values (same pattern), Setup again: a refresh that keeps
    the census, the ordering and the C/F split and takes the new values."""
    A = hc.ij_matrix(mi, M1)
    amg = hierarchy(mi, A, setup_reuse=1)
    assert amg.setup_kind() == (1, 1)
    assert amg.level_value_storage(0, 0)[0] == kind1
    cen, perm, cf = amg.c_row_handover_census(0), amg.level_perm(0), amg.level_cf(0)
    p = perm.astype(np.int64)
    assert abs(hc.level0(amg)[0] - M1[p][:, p]).max() == 0.0
    hc.update_values(A, M2)
    amg.setup(A)
    assert amg.setup_kind()[0] == 2, amg.setup_kind()
    assert amg.c_row_handover_census(0) == cen
    assert np.array_equal(amg.level_perm(0), perm) and np.array_equal(amg.level_cf(0), cf)
    assert amg.level_value_storage(0, 0)[0] == kind2
    M0 = hc.level0(amg)[0]
    assert M0.nnz == M2.nnz and abs(M0 - M2[p][:, p]).max() == 0.0  # the new values, permuted
    r = hc.check_reduced(mi, amg, rhs(M1.shape[0]), raised=True, label=label)
    assert hc.same_bits(r["M"].data, M0.data)
    return amg, r, p


def test_refresh_keeps_the_census_fp64(mi):
    M1, M2 = hc.case("aniso16_8_scaled_nonsym"), hc.scaled(hc.aniso(16, 8), seed=4, sym=False)
    assert np.array_equal(M1.indices, M2.indices) and abs(M1 - M2).max() > 1e-3
    amg, r, p = _refreshed(mi, M1, M2, 0, 0, "refresh: scaled aniso, seed 3 -> 4")
    assert_both_kinds_of_tile(r)


def test_refresh_leaves_the_dictionary(mi):
    M1, M2 = hc.case("aniso22_11"), hc.scaled(hc.aniso(22, 11), seed=3, sym=False)
    assert np.array_equal(M1.indices, M2.indices)
    amg, r, p = _refreshed(mi, M1, M2, 8, 0, "refresh: aniso 22^3 -> scaled")
    assert_both_kinds_of_tile(r)


def test_rows_flagged_by_stored_zeros(mi):
    """The census counts stored entries, zero or not: rows are flagged by pattern, which is what makes it safe for a
    refresh to keep the tile list when those entries take values."""
    M = hc.case("lap7_12")
    amg0 = hierarchy(mi, matrix(mi, "lap7_12"))
    cen0, perm0 = amg0.c_row_handover_census(0), amg0.level_perm(0).astype(np.int64)
    assert cen0["flagged_c_rows"] == 0 and cen0["w_upto"] >= 12
    # 6 pairs of C points of the first handed-over tile, in the caller's numbering
    pairs = [(int(perm0[r]), int(perm0[r + 6])) for r in range(6)]
    touched = sorted(i for pr in pairs for i in pr)
    Z = hc.with_explicit_zeros(M, pairs)
    assert Z.nnz == M.nnz + 12
    D = sp.coo_matrix((np.r_[np.full(12, -0.3), np.full(12, 0.3)],
                       (np.r_[[a for a, b in pairs], [b for a, b in pairs], touched],
                        np.r_[[b for a, b in pairs], [a for a, b in pairs], touched])), shape=M.shape)
    Z2 = (Z + D).tocsr()
    Z2.sort_indices()
    assert np.array_equal(Z2.indptr, Z.indptr) and np.array_equal(Z2.indices, Z.indices)
    for a, b in pairs:
        assert Z2[a, b] == -0.3 and Z2[b, a] == -0.3 and Z2[a, a] == 6.3 and Z2[b, b] == 6.3
    amg, r, p = _refreshed(mi, Z, Z2, 0, 0, "refresh: stored zeros take values")
    assert r["M"].nnz == M.nnz + 12  # the assembly kept the stored zeros
    assert sorted(p[np.flatnonzero(r["flagged"])].tolist()) == touched  # exactly those 12 rows
    assert r["census"]["flagged_c_rows"] == 12 and r["census"]["handed"] > 0


# ---------------------------------------------------------------------------------------------------- (g) Krylov loops
def krylov(mi, A, bs, m, solver="GMRES", kspace=50, max_iterations=100, keep=True, x0=None, converges=True):
    """One solve per right-hand side of bs on the same solver objects in hand-over mode m: a list of
    dict(rc, iters, hist, x, handed)."""
    n = len(bs[0])
    mi.set_c_row_handover(m)
    mi.set_gmres_keep_directions(keep)
    b = mi.IJVector(0, n - 1, bs[0])
    x = mi.IJVector(0, n - 1, np.zeros(n) if x0 is None else x0)
    amg = mi.BoomerAMG(print_level=0)
    ks = getattr(mi, solver)(tolerance=1e-10, max_iterations=max_iterations, kspace=kspace, print_level=0)
    ks.set_precond(amg)
    ks.setup(A, b, x)
    out = []
    for j, bv in enumerate(bs):
        if j:
            b.set(bv)
            x.set(np.zeros(n))
        h0 = mi.counter("handover_matvecs")
        rc = ks.solve(A, b, x)
        assert (rc == 0) == converges, rc
        out.append(dict(rc=rc, iters=ks.num_iterations, hist=np.asarray(ks.residual_history()), x=x.get(),
                        handed=mi.counter("handover_matvecs") - h0))
    return out


def assert_modes_agree(runs, label, handed_in_mode_1=None):
    """runs[m]: krylov()'s list for mode m.  The same iterations, histories to rtol 1e-9, x to 1e-12 (x is about 1: the
    paths differ in the summation order of some rows of w), one reduced mat-vec per iteration in mode 2, none in mode 0."""
    for j in range(len(runs[0])):
        r0 = runs[0][j]
        for m in (1, 2):
            r = runs[m][j]
            dx = np.abs(r["x"] - r0["x"]).max()
            print(f"{label} solve {j} mode {m}: {r['iters']} iterations, {r['handed']} reduced mat-vecs, max|x - x_0| {dx:.3e}")
            assert r["rc"] == r0["rc"] and r["iters"] == r0["iters"]
            assert len(r["hist"]) == len(r0["hist"]) and np.allclose(r["hist"], r0["hist"], rtol=1e-9, atol=0.0)
            assert dx <= 1e-12
        assert r0["handed"] == 0
        assert runs[2][j]["handed"] == runs[2][j]["iters"]
        if handed_in_mode_1 is not None:
            assert runs[1][j]["handed"] == (runs[1][j]["iters"] if handed_in_mode_1 else 0)


VARIANTS = {
    "restarts": dict(kspace=4),
    "flexgmres": dict(solver="FlexGMRES"),
    "cogmres": dict(solver="COGMRES"),
    "directions_recomputed": dict(keep=False),
    "initial_guess": dict(x0=True),
    "cut_at_3": dict(max_iterations=3, converges=False),
    "two_solves": dict(second=True),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", ["lap7_12", "aniso16_8_scaled_nonsym", "lap7_22"])  # fp64, fp64, dictionary
def test_krylov_loops_agree_across_modes(mi, name, variant):
    A, M = matrix(mi, name), hc.case(name)
    n = M.shape[0]
    kw = dict(VARIANTS[variant])
    bs = [M @ np.ones(n)]
    if kw.pop("second", False):
        bs.append(M @ (1.0 + 0.5 * np.random.default_rng(11).random(n)))
    if kw.pop("x0", False):
        kw["x0"] = 0.5 + 0.1 * np.random.default_rng(7).random(n)
    runs = {m: krylov(mi, A, bs, m, **kw) for m in (0, 1, 2)}
    assert_modes_agree(runs, f"{name} {variant}")
    if variant == "restarts":
        assert runs[0][0]["iters"] > 4
    if variant == "cut_at_3":
        assert runs[2][0]["iters"] == 3 and runs[2][0]["handed"] == 3
    for j, bv in enumerate(bs):  # and the solves solve
        if kw.get("converges", True):
            for m in (0, 1, 2):
                assert np.linalg.norm(bv - M @ runs[m][j]["x"]) <= 2e-10 * np.linalg.norm(bv)


def test_threshold_in_a_solve(mi):
    A, M = matrix(mi, "aniso16_4"), hc.case("aniso16_4")
    bs = [M @ np.ones(M.shape[0])]
    runs = {m: krylov(mi, A, bs, m) for m in (0, 1, 2)}
    assert_modes_agree(runs, "aniso16_4", handed_in_mode_1=False)


def test_stale_hierarchy_takes_the_full_matvec(mi):
    """The values change after Setup without a new Setup: the loop no longer runs in the hierarchy's ordering, level 0's
    copy and its tile list are of the old operator and must not serve the mat-vec of the new one."""
    M1, M2 = hc.scaled(hc.lap7(12), seed=3), hc.scaled(hc.lap7(12), seed=4)
    n = M1.shape[0]
    A = hc.ij_matrix(mi, M1)
    bv = M2 @ np.ones(n)
    mi.set_c_row_handover(2)
    b, x = mi.IJVector(0, n - 1, bv), mi.IJVector(0, n - 1, np.zeros(n))
    amg = mi.BoomerAMG(print_level=0)
    gm = mi.GMRES(tolerance=1e-10, max_iterations=100, kspace=50, print_level=0)
    gm.set_precond(amg)
    gm.setup(A, b, x)
    assert amg.c_row_handover_census(0)["handed"] > 0
    stamp = mi.assembly_stamp(A)
    hc.update_values(A, M2)
    assert mi.assembly_stamp(A) != stamp
    h0 = mi.counter("handover_matvecs")
    assert gm.solve(A, b, x) == 0
    assert mi.counter("handover_matvecs") == h0
    res = np.linalg.norm(bv - M2 @ x.get()) / np.linalg.norm(bv)
    print(f"stale hierarchy: {gm.num_iterations} iterations, true relative residual {res:.3e}")
    assert res <= 2e-10
