"""GPU: the device setup kernels, the smoothers and the solve on operators that are NOT M-matrices (tests/systems.py:
mixed_sign_system; the branch conditions are asserted in tests/test_mixed_sign_spec.py) -- negative diagonals select the
mirrored strength rule (strength_k), the sign handling of the interpolation kernels (interp_group_k: the sign of a
strong F neighbour's diagonal, entries of the neighbour's row with the diagonal's sign, zero distribution sums,
special F points) and the signed l1 norms (level_norms_k) that every l1 smoother divides by.

Bars: hierarchies bit for bit against the oracle (tests/test_gpu_setup_kernels.py); one relaxation call
1e-12 * max(1, max|ref|) (tests/test_gpu_amg.py); and bit equality under negation of the whole system: every kernel's
summation order depends on the pattern alone and IEEE rounding is symmetric in sign."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests.agg2s_common import host_amg, ij_host
from tests.systems import MIXED_SIGN_CASES
from tests.test_gpu_agg2s import _assert_bit_identical
from tests.test_gpu_amg import _allclose_ref, _chunk
from tests.test_gpu_setup_kernels import _assert_same_hierarchy
from tests.test_mixed_sign_spec import _bits, _id, full_l1_reference, library_kw, oracle_kw, system

pytestmark = pytest.mark.gpu

TEN = MIXED_SIGN_CASES[1]       # 10 entries per row, 30 % negative diagonals, 25 % positive couplings
ALL_NEG = MIXED_SIGN_CASES[5]   # every diagonal negative (an M-matrix times -1)
POS_OFF = MIXED_SIGN_CASES[6]   # positive diagonals, 35 % positive couplings: the operator of the solves

SETUP_CASES = [(c, kw) for c in MIXED_SIGN_CASES
               for kw in ({}, dict(interp_type=0), dict(trunc_factor=0.2, true_pmax_elmts=0))]
SETUP_CASES += [(TEN, kw) for kw in (dict(coarsen_type=10), dict(coarsen_type=6), dict(agg_num_levels=1),
                                     dict(non_galerkin_tol=0.05), dict(interp_type=3), dict(max_row_sum=0.6),
                                     dict(max_row_sum=0.6, interp_type=0))]


def _device_setup(mi, M, kw, devmin="0"):
    """BoomerAMG set up on the device copy of M; devmin "0": every level built by the device kernels, None: the
    library's threshold (these operators are then set up on the host and uploaded)"""
    old = os.environ.get("MI_HYPRE_DEVICE_SETUP_MIN_ROWS")
    if devmin is None:
        os.environ.pop("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", None)
    else:
        os.environ["MI_HYPRE_DEVICE_SETUP_MIN_ROWS"] = devmin
    try:
        A = mi.matrix_from_scipy(M)
        amg = mi.BoomerAMG(print_level=0, **library_kw(kw))
        amg.setup(A)
    finally:
        if old is None:
            os.environ.pop("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", None)
        else:
            os.environ["MI_HYPRE_DEVICE_SETUP_MIN_ROWS"] = old
    return A, amg


def _oracle(mi, oc, M, kw):
    return oc.Amg(oc.Csr.from_scipy(M), oc.default_params(gs_chunk=_chunk(mi), **oracle_kw(kw)))


@pytest.mark.parametrize("case,kw", SETUP_CASES, ids=_id)
def test_device_setup_equals_oracle(mi, oc, case, kw, monkeypatch):
    """A, P, R and the marks of every level built by the device kernels, bit for bit; rows of 4 to 89 entries: every
    lanes-per-row instantiation of the strength, norm and product kernels.  Of the interpolation kernel only the tables
    of up to 128 entries run here (the bound of a row stays below 105): tests/test_gpu_interp_tables.py has the rest."""
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    M = system(case)
    A = mi.matrix_from_scipy(M)
    amg = mi.BoomerAMG(print_level=0, **library_kw(kw))
    amg.setup(A)
    oamg = _oracle(mi, oc, M, kw)
    assert amg.num_levels > 1
    _assert_same_hierarchy(amg, oamg)


_hierarchies = {}


def _hierarchy(mi, oc, case, devmin, sign=1):
    """(A, amg, oracle amg) of sign * the case's operator, default parameters, built once per module run"""
    key = (case, devmin, sign)
    if key not in _hierarchies:
        M = system(case) if sign > 0 else (-system(case)).tocsr()
        A, amg = _device_setup(mi, M, {}, devmin)
        _hierarchies[key] = (A, amg, _oracle(mi, oc, M, {}))
    return _hierarchies[key]


@pytest.mark.parametrize("devmin", ["0", None], ids=["device-setup", "host-setup"])
@pytest.mark.parametrize("case", [TEN, ALL_NEG, MIXED_SIGN_CASES[3]], ids=_id)
def test_level_norms_equal_oracle(mi, oc, case, devmin):
    """the signed l1 norms of every level (level_norms_k on the device, the host routine otherwise), bit for bit"""
    A, amg, oamg = _hierarchy(mi, oc, case, devmin)
    assert amg.num_levels == oamg.num_levels
    for l in range(amg.num_levels):
        diag, l1gs, l1jac = amg.level_norms(l)
        Al = oamg.level_A(l).to_scipy().tocsr()
        assert np.array_equal(_bits(diag), _bits(Al.diagonal())), l
        assert np.array_equal(_bits(l1gs), _bits(oamg.level_l1(l))), l
        assert np.array_equal(_bits(l1jac), _bits(full_l1_reference(Al))), l
        if l == 1:
            assert (diag < 0).any()


@pytest.mark.parametrize("rtype", [0, 3, 4, 6, 7, 8, 13, 14, 18, 11])
@pytest.mark.parametrize("devmin", ["0", None], ids=["device-setup", "host-setup"])
@pytest.mark.parametrize("case", [TEN, ALL_NEG], ids=_id)
def test_relax_matches_oracle(mi, oc, case, devmin, rtype):
    """one relaxation call on all / C / F points of levels 0 and 1, and the zero-guess C-then-F pair of the hybrid
    Gauss-Seidel types, against the oracle"""
    A, amg, oamg = _hierarchy(mi, oc, case, devmin)
    assert amg.num_levels == oamg.num_levels and amg.num_levels > 2
    rng = np.random.default_rng(300 + rtype)
    for level in (0, 1):
        Al = oamg.level_A(level).to_scipy()
        assert (Al.diagonal() < 0).mean() >= 0.2  # level 1 still has negative diagonals
        nl = Al.shape[0]
        cf = oamg.level_cf(level)
        assert np.array_equal(amg.level_cf(level), cf)
        f, u0 = rng.standard_normal(nl), rng.standard_normal(nl)
        for points in (0, 1, -1):
            got = amg.relax_level(level, rtype, points, f, u0)
            ref = oamg.relax(level, rtype, points, f, u0)
            err = np.abs(got - ref).max()
            assert err <= 1e-12 * max(1.0, np.abs(ref).max()), (level, points, err)
            if points != 0 and rtype != 11:  # (the two-stage Gauss-Seidel ignores the marker)
                assert np.array_equal(got[cf != points], u0[cf != points])
        if rtype in (3, 4, 6, 8, 13, 14):
            got = amg.relax_pair_level(level, rtype, 1, f)
            ref = oamg.relax(level, rtype, -1, f, oamg.relax(level, rtype, 1, f, np.zeros(nl)))
            assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), level


def assert_mirrored_hierarchies(plus, minus, exact_zeros=None):
    """minus: the device hierarchy of -A, plus: of A -- same marks, the same bits in P and R, A_l and the norms negated.
    exact_zeros (a list, optional): stored entries of A_l that are exactly zero in both hierarchies are exempt from the
    sign -- a Galerkin sum that cancels exactly is +0 whichever sign its terms have, the one case in which IEEE
    addition does not mirror -- and their number per level is appended to the list."""
    assert plus.num_levels == minus.num_levels and plus.num_levels > 1
    for l in range(plus.num_levels):
        ia, ja, a, _ = plus.level_csr(l, 0)
        mia, mja, ma, _ = minus.level_csr(l, 0)
        assert np.array_equal(ia, mia) and np.array_equal(ja, mja), l
        if exact_zeros is not None:
            both = (a == 0.0) & (ma == 0.0)
            exact_zeros.append(int(both.sum()))
            a, ma = a[~both], ma[~both]
        assert np.array_equal(_bits(-ma), _bits(a)), l
        for got, want in zip(minus.level_norms(l), plus.level_norms(l)):
            assert np.array_equal(_bits(-got), _bits(want)), l
        if l < plus.num_levels - 1:
            assert np.array_equal(plus.level_cf(l), minus.level_cf(l)), l
            assert np.array_equal(plus.level_perm(l), minus.level_perm(l)), l
            for which in (2, 3):
                ia, ja, a, _ = plus.level_csr(l, which)
                mia, mja, ma, _ = minus.level_csr(l, which)
                assert np.array_equal(ia, mia) and np.array_equal(ja, mja), (l, which)
                assert np.array_equal(_bits(ma), _bits(a)), (l, which)


@pytest.mark.parametrize("kw", [{}, dict(interp_type=0), dict(trunc_factor=0.2, true_pmax_elmts=0), dict(coarsen_type=10),
                                dict(non_galerkin_tol=0.05), dict(max_row_sum=0.6)], ids=_id)
@pytest.mark.parametrize("case", [TEN, POS_OFF], ids=_id)
def test_device_setup_mirrors_under_negation(mi, case, kw, monkeypatch):
    """the device setup of -A against the device setup of A: same marks, the same bits in P and R, A_l negated"""
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    M = system(case)
    amgs = []
    for Ms in (M, (-M).tocsr()):
        A = mi.matrix_from_scipy(Ms)
        amg = mi.BoomerAMG(print_level=0, **library_kw(kw))
        amg.setup(A)
        amgs.append(amg)
    assert_mirrored_hierarchies(*amgs)


@pytest.mark.parametrize("devmin", ["0", None], ids=["device-setup", "host-setup"])
@pytest.mark.parametrize("case", [TEN, POS_OFF], ids=_id)
def test_relax_mirrors_under_negation(mi, oc, case, devmin):
    """relax_level(-f, u0) on the hierarchy of -A gives the bits of relax_level(f, u0) on the hierarchy of A: every
    smoother, all / C / F points, two levels, and the zero-guess pair"""
    _, plus, _ = _hierarchy(mi, oc, case, devmin)
    _, minus, _ = _hierarchy(mi, oc, case, devmin, sign=-1)
    rng = np.random.default_rng(17)
    for level in (0, 1):
        nl = plus.level_csr(level, 0)[3][0]
        f, u0 = rng.standard_normal(nl), rng.standard_normal(nl)
        for rtype in (0, 3, 4, 6, 7, 8, 13, 14, 18, 11):
            for points in (0, 1, -1):
                a, b = plus.relax_level(level, rtype, points, f, u0), minus.relax_level(level, rtype, points, -f, u0)
                assert np.array_equal(_bits(a), _bits(b)), (level, rtype, points, np.abs(a - b).max())
            if rtype in (3, 4, 6, 8, 13, 14):
                a, b = plus.relax_pair_level(level, rtype, 1, f), minus.relax_pair_level(level, rtype, 1, -f)
                assert np.array_equal(_bits(a), _bits(b)), (level, rtype, "pair")


def _solve(mi, M, bv, devmin, **kw):
    old = os.environ.get("MI_HYPRE_DEVICE_SETUP_MIN_ROWS")
    if devmin is not None:
        os.environ["MI_HYPRE_DEVICE_SETUP_MIN_ROWS"] = devmin
    try:
        n = M.shape[0]
        A = mi.matrix_from_scipy(M)
        b = mi.IJVector(0, n - 1, bv)
        x = mi.IJVector(0, n - 1, np.zeros(n))
        amg = mi.BoomerAMG(print_level=0, **library_kw(kw))
        gm = mi.GMRES(tolerance=1e-8, max_iterations=60, kspace=30, print_level=0)
        gm.set_precond(amg)
        gm.setup(A, b, x)
        rc = gm.solve(A, b, x)
        return dict(rc=rc, iters=gm.num_iterations, hist=np.asarray(gm.residual_history()), x=x.get(), amg=amg)
    finally:
        if old is None:
            os.environ.pop("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", None)
        else:
            os.environ["MI_HYPRE_DEVICE_SETUP_MIN_ROWS"] = old


def _rhs(M):
    return M @ np.random.default_rng(5).standard_normal(M.shape[0])


@pytest.mark.parametrize("devmin", ["0", None], ids=["device-setup", "host-setup"])
def test_gmres_amg_mirrors_under_negation_and_matches_oracle(mi, oc, devmin):
    """GMRES(30) + AMG on (A, b) twice and on (-A, -b): iteration count, residual history and x are the same bits in all
    three runs; and both signs against the oracle's solve with the assertions of
    tests/test_gpu_amg.py::test_seeded_random_systems_match_oracle."""
    M = system(POS_OFF)
    bv = _rhs(M)
    first, again = _solve(mi, M, bv, devmin), _solve(mi, M, bv, devmin)
    mirror = _solve(mi, (-M).tocsr(), -bv, devmin)
    for name, other in (("repeat", again), ("negated", mirror)):
        assert other["iters"] == first["iters"], name
        dh = np.abs(other["hist"] - first["hist"]).max()
        dx = np.abs(other["x"] - first["x"]).max()
        print("%s run: max |history difference| %.3e, max |x difference| %.3e" % (name, dh, dx))
        assert np.array_equal(_bits(other["hist"]), _bits(first["hist"])), (name, dh)
        assert np.array_equal(_bits(other["x"]), _bits(first["x"])), (name, dx)
    for sign, run in ((1.0, first), (-1.0, mirror)):
        Ms = (sign * M).tocsr()
        Ao = oc.Csr.from_scipy(Ms)
        oamg = oc.Amg(Ao, oc.default_params(gs_chunk=_chunk(mi), **oracle_kw({})))
        xo, info = oc.gmres(Ao, sign * bv, kdim=30, tol=1e-8, maxit=60, amg=oamg)
        assert info["rel_res"] <= 1e-8 and info["iters"] <= 10
        assert run["amg"].num_levels == oamg.num_levels
        assert np.array_equal(run["amg"].level_cf(0), oamg.level_cf(0))
        assert run["iters"] == info["iters"], (run["iters"], info["iters"])
        ref = np.asarray(info["norms"])
        assert run["rc"] == 0 and np.allclose(run["hist"], ref, rtol=1e-7, atol=1e-13 * ref[0])
        assert _allclose_ref(run["x"], xo, rtol=1e-5, atol=1e-7)


def test_fp32_value_storage_on_the_negated_operator(mi):
    """HYPRE_MI_BoomerAMGSetValueStorage on -A: mode 1 (fp32 stream) against mode 2 (fp64 stream of the fp32-rounded
    values), the same bits in the residual history and in x; the coarse operators were really narrowed"""
    M = (-system(POS_OFF)).tocsr()
    bv = _rhs(M)
    one = _solve(mi, M, bv, "0", mi_value_storage=1)
    two = _solve(mi, M, bv, "0", mi_value_storage=2)
    assert one["amg"].level_value_storage(1, 0)[0] == 1 and two["amg"].level_value_storage(1, 0)[0] == 2
    assert one["rc"] == 0 and one["iters"] == two["iters"]
    assert np.array_equal(_bits(one["hist"]), _bits(two["hist"])) and np.array_equal(_bits(one["x"]), _bits(two["x"]))
    assert np.linalg.norm(bv - M @ one["x"]) <= 2e-8 * np.linalg.norm(bv)


def test_two_stage_aggressive_interpolation_device_equals_host(mi, monkeypatch):
    """agg_num_levels 1 with agg_interp_type 5 on the operator with 30 % negative diagonals and 25 % positive couplings:
    the device setup against the host-only setup, bit for bit (the host side against its restatement:
    tests/test_mixed_sign_spec.py; no row has a zero denominator there)"""
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    monkeypatch.setenv("MI_HYPRE_LOCALITY_ORDER", "0")
    M = system(TEN)
    kw = library_kw(dict(agg_num_levels=1, agg_interp_type=5))
    A = mi.matrix_from_scipy(M)
    dev = mi.BoomerAMG(print_level=0, keep_agg_markers=1, **kw)
    dev.setup(A)
    host = host_amg(mi, ij_host(mi, M), **kw)
    _assert_bit_identical(dev, host, 1)
