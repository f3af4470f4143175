"""CPU: AMG setup and relaxation on operators that are NOT M-matrices (tests/systems.py: mixed_sign_system) -- negative
diagonals, positive couplings, rows over max_row_sum, special F points.  Three independent statements of one
specification are held against each other: the plain-Python formulas of tests/interp_ref.py, the oracle, and the
library's host setup (HYPRE_MI_BoomerAMGSetupHostOnly); and both setups against themselves under negation of the whole
system, which must mirror every level bit for bit (IEEE rounding is symmetric in sign and no summation order depends on
a value)."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.agg2s_common import ij_host
from tests.agg2s_ref import strength_rows
from tests.interp_ref import (classical_modified_reference, extended_i_reference, special_f_points, strength_pattern)
from tests.systems import MIXED_SIGN_CASES, mixed_sign_system

THETA = 0.25  # the threshold at which the operators of MIXED_SIGN_CASES were chosen (3 to 5 levels, no zero diagonal)

# BoomerAMG choices of the setup comparisons (library keys); every one but the last two on top of strong_threshold 0.25
SETUP_PARAMS = [{}, dict(interp_type=0), dict(trunc_factor=0.2), dict(coarsen_type=10), dict(coarsen_type=6),
                dict(agg_num_levels=1), dict(interp_type=3), dict(interp_type=4), dict(non_galerkin_tol=0.05),
                dict(max_row_sum=0.6), dict(max_row_sum=0.6, interp_type=0),
                dict(strong_threshold=0.57), dict(strong_threshold=0.57, interp_type=0)]


def _id(v):
    if isinstance(v, dict):
        return "-".join("%s=%s" % kv for kv in v.items()) or "default"
    return "-".join(str(x) for x in v)


def library_kw(kw):
    return dict(dict(strong_threshold=THETA), **kw)


def oracle_kw(kw):
    """the oracle's names of the library's keys"""
    okw = {("pmax_elmts" if k == "true_pmax_elmts" else k): v for k, v in library_kw(kw).items()}
    if "non_galerkin_tol" in okw:  # one tolerance per fine level there
        okw["non_galerkin_tol"] = [okw["non_galerkin_tol"]] * 12
    return okw


_systems = {}


def system(case):
    """the seeded operator of a case, built once; callers do not modify it"""
    if case not in _systems:
        _systems[case] = mixed_sign_system(*case)
    return _systems[case]


# ---------------------------------------------------------------------------------------------------------------
# the oracle against the plain-Python formulas
# ---------------------------------------------------------------------------------------------------------------
# (n, seed, flip_rows, pos_frac, per, symmetric_pattern)
SPEC_CASES = [(600, 100 + 10 * a + b, fl, pf, (1.5, 3.0, 6.0)[(a + b) % 3], True)
              for a, fl in enumerate((0, 0.3, 0.5, 1.0)) for b, pf in enumerate((0, 0.25, 0.45))]
SPEC_CASES.append((600, 171, 0.3, 0.25, 3.0, False))


def _zero_sum_neighbours_classical(A, strong, cf):
    """strong F-F pairs (i, k) of F rows with a C neighbour where k has no entry of the distributing sign in C_i"""
    A = sp.csr_matrix(A)
    rows = [dict(zip(A.indices[A.indptr[i]:A.indptr[i + 1]], A.data[A.indptr[i]:A.indptr[i + 1]])) for i in range(A.shape[0])]
    count = 0
    for i in np.flatnonzero(cf != 1):
        Ci = [j for j in strong[i] if cf[j] == 1]
        if not Ci:
            continue
        for k in strong[i]:
            if cf[k] != 1 and len(strong[k]) and not any(rows[k].get(m, 0.0) * rows[k][k] < 0 for m in Ci):
                count += 1
    return count


@pytest.mark.parametrize("case", SPEC_CASES, ids=_id)
def test_oracle_matches_the_published_formulas(oc, case):
    """Level-0 P without truncation, extended+i and classical modified, theta 0.25 / 0.5, max_row_sum 0.6 / 0.9 / 1.0:
    the oracle against tests/interp_ref.py to 1e-13 (2.8e-16 was measured).  The branch conditions this module exists
    for are asserted from the matrix, the strength rows and the oracle's C/F marks alone."""
    n, seed, flip_rows, pos_frac, per, symmetric = case
    M = mixed_sign_system(n, seed, flip_rows, pos_frac, per, symmetric_pattern=symmetric)
    d = M.diagonal()
    off = (M - sp.diags(d)).tocsr()
    off.eliminate_zeros()
    assert np.all(d != 0.0)
    if flip_rows >= 0.3:
        assert (d < 0).mean() >= 0.2
    if flip_rows == 0:
        assert np.all(d > 0)
    if pos_frac >= 0.25:
        sign_of_diag = np.repeat(np.sign(d), np.diff(off.indptr))
        assert (off.data * sign_of_diag > 0).mean() >= 0.2  # couplings with the diagonal's sign
    Ao = oc.Csr.from_scipy(M)
    worst = 0.0
    seen = dict(special_f=0, over_row_sum=0, zero_sum_classical=0, zero_sum_extended=0)
    for theta in (0.25, 0.5):
        for mrs in (0.6, 0.9, 1.0):
            strong = strength_rows(M, theta, mrs)
            has_off = np.diff(off.indptr) > 0
            over = np.abs(np.asarray(M.sum(axis=1)).ravel()) > np.abs(d) * mrs
            if mrs < 1.0:  # rows over max_row_sum keep no strong connection
                seen["over_row_sum"] += int((over & has_off).sum())
                assert all(len(strong[i]) == 0 for i in np.flatnonzero(over))
            for interp in (6, 0):
                amg = oc.Amg(Ao, oc.default_params(pmax_elmts=0, interp_type=interp, strong_threshold=theta, max_row_sum=mrs))
                assert amg.num_levels > 1
                Al = amg.level_A(0).to_scipy().tocsr()
                Al.sort_indices()
                cf = np.asarray(amg.level_cf(0))
                S = strength_pattern(Al, theta, mrs)
                census = {}
                ref = extended_i_reference if interp == 6 else classical_modified_reference
                Pref = ref(Al, S, cf, census).tocsc()[:, np.asarray(amg.level_perm(1))].tocsr()
                Po = amg.level_P(0).to_scipy().tocsr()
                assert Po.shape == Pref.shape
                err = abs(Po - Pref).max()
                worst = max(worst, err)
                assert err < 1e-13, (theta, mrs, interp, err)
                # special F points that are strong neighbours of an F row with an interpolatory set: from the strength
                # graph and the marks (not from the census of the formulas, which only has to agree)
                sl = [set(S.indices[S.indptr[i]:S.indptr[i + 1]]) for i in range(n)]
                special = special_f_points(S, cf)
                hit = sum(1 for i in np.flatnonzero(cf != 1) if any(cf[j] == 1 for j in sl[i])
                          for k in sl[i] if special[k])
                seen["special_f"] += hit
                if interp == 0:
                    assert census["special_f"] == hit
                    zs = _zero_sum_neighbours_classical(Al, sl, cf)
                    assert census["zero_sum"] == zs
                    seen["zero_sum_classical"] += zs
                else:
                    seen["zero_sum_extended"] += census["zero_sum"]
    print("max |P_oracle - P_formula| = %.2e, branch census %s" % (worst, seen))
    assert seen["zero_sum_classical"] >= 1
    # without positive couplings the row sum stays below 0.2 / 1.2 of the diagonal and the largest coupling of a row is
    # always strong: rows over max_row_sum and special F points need pos_frac > 0
    if pos_frac >= 0.25:
        assert seen["over_row_sum"] >= 1
        assert seen["special_f"] >= 1


# ---------------------------------------------------------------------------------------------------------------
# the library's host setup against the oracle, and both against themselves under negation
# ---------------------------------------------------------------------------------------------------------------
def host_setup(mi, M, kw):
    A = ij_host(mi, M)
    amg = mi.BoomerAMG(print_level=0, **library_kw(kw))
    mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
    return amg


def oracle_setup(oc, M, kw, **more):
    return oc.Amg(oc.Csr.from_scipy(M), oc.default_params(**oracle_kw(kw), **more))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def library_levels(amg):
    """[(A ia, ja, a, cf, perm, P ia, ja, a)] of a library hierarchy (cf .. P a: None on the coarsest level)"""
    out = []
    for l in range(amg.num_levels):
        ia, ja, a, _ = amg.level_csr(l, 0)
        if l < amg.num_levels - 1:
            pia, pja, pa, _ = amg.level_csr(l, 2)
            out.append((ia, ja, a, amg.level_cf(l), amg.level_perm(l), pia, pja, pa))
        else:
            out.append((ia, ja, a, None, None, None, None, None))
    return out


def oracle_levels(oamg):
    out = []
    for l in range(oamg.num_levels):
        ia, ja, a = oamg.level_A(l).arrays()
        if l < oamg.num_levels - 1:
            pia, pja, pa = oamg.level_P(l).arrays()
            out.append((ia, ja, a, oamg.level_cf(l), oamg.level_perm(l), pia, pja, pa))
        else:
            out.append((ia, ja, a, None, None, None, None, None))
    return out


def assert_levels_equal(got, want, negated=False):
    """bit-equal ia, ja, values, marks, permutation and P on every level; negated: `got` belongs to the negated system,
    whose operators are the negatives and whose marks, permutations and interpolation are the same"""
    assert len(got) == len(want)
    for l, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), l
        assert np.array_equal(_bits(-g[2] if negated else g[2]), _bits(w[2])), l
        if w[3] is None:
            assert g[3] is None
            continue
        assert np.array_equal(g[3], w[3]), l
        assert np.array_equal(g[4], w[4]), l
        assert np.array_equal(g[5], w[5]) and np.array_equal(g[6], w[6]), l
        assert np.array_equal(_bits(g[7]), _bits(w[7])), l


@pytest.mark.parametrize("kw", SETUP_PARAMS, ids=_id)
@pytest.mark.parametrize("case", MIXED_SIGN_CASES, ids=_id)
def test_host_setup_equals_oracle_and_mirrors_under_negation(mi_lib, oc, case, kw):
    """Every level of the host-only setup equals the oracle's bit for bit (ia, ja, values, marks, permutation, P), for
    A and for -A; and the hierarchy of -A is the mirror image of the hierarchy of A -- same marks, the same bits in P,
    A_l negated -- in the oracle and in the library.  Direct interpolation (interp_type 3) is not mirror-symmetric (it
    lumps on sum_P_pos == 0 alone, like the routine it restates): there only the equality with the oracle is asserted,
    on both signs."""
    M = system(case)
    Mn = (-M).tocsr()
    plus, minus = oracle_levels(oracle_setup(oc, M, kw)), oracle_levels(oracle_setup(oc, Mn, kw))
    assert len(plus) >= 2
    if kw in ({}, dict(interp_type=0)):
        assert 3 <= len(plus) <= 5
    for lv in plus:
        assert np.all(np.isfinite(lv[2]))
    if case[2] >= 0.3 and len(plus) > 2 and "agg_num_levels" not in kw:
        ia, ja, a = plus[1][:3]
        d1 = sp.csr_matrix((a, ja, ia)).diagonal()
        assert (d1 < 0).any() and np.all(d1 != 0)  # the coarse levels keep negative diagonals
    lib_plus = library_levels(host_setup(mi_lib, M, kw))
    lib_minus = library_levels(host_setup(mi_lib, Mn, kw))
    assert_levels_equal(lib_plus, plus)
    assert_levels_equal(lib_minus, minus)
    if kw.get("interp_type") != 3:
        assert_levels_equal(minus, plus, negated=True)
        assert_levels_equal(lib_minus, lib_plus, negated=True)


@pytest.mark.parametrize("case", [MIXED_SIGN_CASES[1], MIXED_SIGN_CASES[2], MIXED_SIGN_CASES[6]], ids=_id)
def test_oracle_relaxation_and_solve_mirror_under_negation(oc, case):
    """relax(-f, u0) on the hierarchy of -A gives the bits of relax(f, u0) on the hierarchy of A (every smoother, all /
    C / F points, two levels: the l1 norms carry the diagonal's sign), and GMRES + AMG on (-A, -b) reproduces the
    residual history and the solution of (A, b)."""
    M = system(case)
    n = M.shape[0]
    plus, minus = oracle_setup(oc, M, {}), oracle_setup(oc, (-M).tocsr(), {})
    rng = np.random.default_rng(case[1])
    for level in (0, 1):
        nl = plus.level_A(level).shape[0]
        l1p, l1m = plus.level_l1(level), minus.level_l1(level)
        dl = plus.level_A(level).to_scipy().diagonal()
        assert np.array_equal(_bits(-l1m), _bits(l1p)) and np.all(np.sign(l1p) == np.sign(dl))
        assert np.all(np.abs(l1p) >= np.abs(dl))
        f, u0 = rng.standard_normal(nl), rng.standard_normal(nl)
        for rtype in (0, 3, 6, 7, 8, 11, 13, 14, 18):
            for points in (0, 1, -1):
                a, b = plus.relax(level, rtype, points, f, u0), minus.relax(level, rtype, points, -f, u0)
                assert np.array_equal(_bits(a), _bits(b)), (level, rtype, points)
                assert not np.array_equal(a, u0)
    bv = M @ rng.standard_normal(n)
    Ap, Am = oc.Csr.from_scipy(M), oc.Csr.from_scipy((-M).tocsr())
    xp, ip = oc.gmres(Ap, bv, kdim=30, tol=1e-8, maxit=40, amg=plus)
    xm, im = oc.gmres(Am, -bv, kdim=30, tol=1e-8, maxit=40, amg=minus)
    assert ip["iters"] == im["iters"] and ip["iters"] > 0
    assert np.array_equal(_bits(ip["norms"]), _bits(im["norms"])) and np.array_equal(_bits(xp), _bits(xm))
    if case[2] == 0:  # positive diagonals with 35 % positive couplings: the solve the device tests repeat
        assert ip["converged"] and ip["iters"] <= 10


def full_l1_reference(A):
    """sign(a_ii) * sum_j |a_ij|, the terms added one after the other in stored order"""
    A = sp.csr_matrix(A)
    out = np.zeros(A.shape[0])
    for i in range(A.shape[0]):
        s = 0.0
        for v in A.data[A.indptr[i]:A.indptr[i + 1]]:
            s += abs(v)
        out[i] = -s if A[i, i] < 0 else s
    return out


@pytest.mark.parametrize("case", [MIXED_SIGN_CASES[0], MIXED_SIGN_CASES[3], MIXED_SIGN_CASES[5]], ids=_id)
def test_host_level_norms_carry_the_sign_of_the_diagonal(mi_lib, oc, case):
    """What the l1 smoothers (relax types 7, 8, 13, 14, 18) divide by, on every level of the host setup: the chunk l1
    norm equals the oracle's bit for bit, the full l1 norm equals its definition, both have the diagonal's sign and at
    least its size, and negating the system negates them."""
    mi = mi_lib
    M = system(case)
    chunk = mi.c_int()
    mi.call("HYPRE_MI_GetGSChunk", mi.C.byref(chunk))
    oamg = oracle_setup(oc, M, {}, gs_chunk=chunk.value)
    plus, minus = host_setup(mi, M, {}), host_setup(mi, (-M).tocsr(), {})
    assert plus.num_levels == oamg.num_levels
    negative = 0
    for l in range(plus.num_levels):
        diag, l1gs, l1jac = plus.level_norms(l)
        Al = oamg.level_A(l).to_scipy().tocsr()
        assert np.array_equal(_bits(diag), _bits(Al.diagonal()))
        assert np.array_equal(_bits(l1gs), _bits(oamg.level_l1(l))), l
        assert np.array_equal(_bits(l1jac), _bits(full_l1_reference(Al))), l
        assert np.all(np.sign(l1gs) == np.sign(diag)) and np.all(np.sign(l1jac) == np.sign(diag))
        assert np.all(np.abs(l1gs) >= np.abs(diag)) and np.all(np.abs(l1jac) >= np.abs(l1gs))
        negative += int((diag < 0).sum()) if l > 0 else 0
        for got, want in zip(minus.level_norms(l), (diag, l1gs, l1jac)):
            assert np.array_equal(_bits(-got), _bits(want)), l
    assert negative > 0  # (negative diagonals on the coarse levels too)


@pytest.mark.parametrize("case", [MIXED_SIGN_CASES[0], MIXED_SIGN_CASES[1], MIXED_SIGN_CASES[5]], ids=_id)
def test_two_stage_aggressive_interpolation_equals_its_restatement(mi_lib, case):
    """agg_interp_type 5 on an aggressive level 0 of the host setup against tests/agg2s_ref.py (which takes the signs as
    they come: strength by the mirrored rule, no sign test in the formula).  No row of these operators has a zero
    denominator with a non-empty numerator -- the restatement would raise and the library would refuse the setup."""
    from tests import agg2s_ref
    from tests.agg2s_common import host_amg
    from tests.test_agg2s_spec import natural_level, same_pattern_close_values

    M = system(case)
    amg = host_amg(mi_lib, ij_host(mi_lib, M), agg_num_levels=1, agg_interp_type=5, strong_threshold=THETA)
    assert amg.num_levels >= 2
    A, m1, m2, P = natural_level(amg, 0)
    assert (A.diagonal() < 0).mean() >= 0.2
    if case[3] > 0:
        assert (m1 == -3).any()  # special F points of the first stage
    Pref = agg2s_ref.two_stage(A, agg2s_ref.strength_rows(A, THETA), m1, m2)
    same_pattern_close_values(P, Pref)
