"""GPU: the approximate ideal restriction (HYPRE_BoomerAMGSetRestriction 1) and the one-point interpolation
(interp_type 100) on the device, through the C ABI -- the two ...Op entries against the host
routines bit for bit on every case of tests/air_cases.py, the fallback and the singular neighbourhood, whole hierarchies
against the host-only setup, the two-level method as a solver against the numpy cycle, GMRES + AMG, the driver and
setup reuse."""
import os
import re

import numpy as np
import pytest

from tests import air_cases as ac
from tests import air_ref as ref
from tests import mm_interp_ref
from tests.agg2s_common import csr, host_amg, ij_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def device_matrix(mi, M):
    A = mi.IJMatrix(0, M.shape[0] - 1)
    coo = M.tocoo()
    A.set_values_coo(coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data.astype(np.float64))
    A.assemble()
    return A


def device_vector(mi, v):
    return mi.IJVector(0, len(v) - 1, np.ascontiguousarray(v, dtype=np.float64))


@pytest.mark.parametrize("name", list(ac.kernel_cases()))
def test_device_restriction_has_the_bits_of_the_host_routine(mi, name):
    A, cf, th, phi = ac.kernel_cases()[name]
    Rd, di = mi.air_restriction_op(A, cf, th, phi)
    Rh, hi = mi.air_restriction_op(A, cf, th, phi, host=True)
    assert di["status"] == 0 and ac.same_bits(Rd, Rh)
    for key in ("max_m", "zero_rows", "dropped", "bad_row"):
        assert di[key] == hi[key], key
    nc = int((cf == 1).sum())
    assert di["rows16"] + di["rows32"] + di["rows64"] == nc and hi["rows16"] + hi["rows32"] + hi["rows64"] == 0
    lens = np.array([len(v) for v in ref.neighbourhoods(A, cf, th)])
    want = [int((lens <= 16).sum()), int(((lens > 16) & (lens <= 32)).sum()), int((lens > 32).sum())]
    assert [di["rows16"], di["rows32"], di["rows64"]] == want
    if name.startswith("hubs"):  # every instantiation of the solve ran, on both sides of its boundary
        assert min(want) >= 2 and {16, 17, 32, 33, 64} <= set(lens.tolist())


def test_a_65_point_neighbourhood_is_left_to_the_host_routine(mi):
    A, cf, hubs = ac.hub_case(ac.GROUP_LENGTHS + (ac.FALLBACK_LENGTH,), 3)
    R, info = mi.air_restriction_op(A, cf)
    assert R is None and info["status"] == 1 and info["max_m"] == ac.FALLBACK_LENGTH
    R, info = mi.air_restriction_op(A, cf, host=True)
    assert R is not None and info["status"] == 0 and info["max_m"] == ac.FALLBACK_LENGTH


def test_the_singular_neighbourhood_reports_its_row(mi):
    M, gadget = ac.singular_case()
    cf = -np.ones(M.shape[0], dtype=np.int32)
    cf[:60:2] = 1
    cf[ac.SINGULAR_ROW] = 1
    with pytest.raises(mi.HypreError, match=r"row %d has a singular local system" % ac.SINGULAR_ROW) as e:
        mi.air_restriction_op(M, cf)
    assert e.value.info["status"] == 2 and e.value.info["bad_row"] == ac.SINGULAR_ROW
    mi.call("HYPRE_ClearAllErrors")


def test_device_one_point_interpolation_has_the_bits_of_the_host_routine(mi):
    A, strong, cf = ac.one_point_case()
    S = ac.strong_csr(strong, 6)
    P = mi.one_point_interp_op(A, S, cf)
    assert ac.same_bits(P, mi.one_point_interp_op(A, S, cf, host=True))
    assert list(P[1]) == [0, 1, 2, 0, 2] and list(np.diff(P[0])) == [1, 1, 1, 1, 1, 0]  # the tie, and the empty row
    for name in ("hubs", "upwind12_pe0.6", "upwind8_pe1000"):
        A, cf, _, _ = ac.kernel_cases()[name]
        strong = mm_interp_ref.strength_rows(A, 0.25)
        S = ac.strong_csr(strong, A.shape[0])
        P = mi.one_point_interp_op(A, S, cf)
        assert ac.same_bits(P, mi.one_point_interp_op(A, S, cf, host=True)), name
        want = ref.one_point_interp(A, strong, cf)
        assert np.array_equal(P[0], want.indptr) and np.array_equal(P[1], want.indices) and np.array_equal(P[2], want.data)
        assert (np.diff(P[0]) == 0).sum() > 0  # F rows without a strong C point


def _assert_hierarchies_have_the_same_bits(dev, host):
    assert dev.num_levels == host.num_levels and dev.num_levels > 2
    for l in range(dev.num_levels):
        for which in (0, 2, 3) if l < dev.num_levels - 1 else (0,):
            assert ac.same_bits(dev.level_csr(l, which), host.level_csr(l, which)), (l, which)
        if l < dev.num_levels - 1:
            assert np.array_equal(dev.level_cf(l), host.level_cf(l)), l
            assert np.array_equal(dev.level_perm(l), host.level_perm(l)), l


@pytest.mark.parametrize("interp", [100, 6])
@pytest.mark.parametrize("pe", [1000, 0.6])
def test_device_hierarchy_has_the_bits_of_the_host_only_setup(mi, pe, interp, monkeypatch):
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    monkeypatch.setenv("MI_HYPRE_LOCALITY_ORDER", "0")
    M = ac.upwind_constant(12, pe)
    kw = dict(restriction=1, interp_type=interp)
    dev = mi.BoomerAMG(print_level=0, **kw)
    A = device_matrix(mi, M)
    dev.setup(A)
    host = host_amg(mi, ij_host(mi, M), **kw)
    _assert_hierarchies_have_the_same_bits(dev, host)
    for l in range(dev.num_levels - 1):
        d, h = dev.restriction_info(l), host.restriction_info(l)
        assert d["kind"] == 1 and h["kind"] == 2, (l, d, h)  # the device built them
        assert {k: d[k] for k in ("max_m", "zero_rows", "dropped")} == {k: h[k] for k in ("max_m", "zero_rows", "dropped")}


def test_device_hierarchy_with_the_filter_and_with_restriction_0(mi, monkeypatch):
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    monkeypatch.setenv("MI_HYPRE_LOCALITY_ORDER", "0")
    M = ac.upwind_constant(12, 0.6)
    for kw in (dict(restriction=1, interp_type=100, filter_threshold_r=0.9, strong_threshold_r=0.1), dict(interp_type=100)):
        dev = mi.BoomerAMG(print_level=0, **kw)
        A = device_matrix(mi, M)
        dev.setup(A)
        _assert_hierarchies_have_the_same_bits(dev, host_amg(mi, ij_host(mi, M), **kw))
        info = dev.restriction_info(0)
        assert (info["kind"], info["dropped"] > 0) == ((1, True) if "restriction" in kw else (0, False))


def test_device_levels_above_host_levels(mi, monkeypatch):
    """The threshold between two level sizes (1728, 890 | 401, 145, 45, 3 rows): levels 0 and 1 are built by the device,
    the others by the host routines, so the C-first renumbering permutes the device's R of level 1 by the host-resident
    order of level 2."""
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "500")
    monkeypatch.setenv("MI_HYPRE_LOCALITY_ORDER", "0")
    M = ac.upwind_constant(12, 1000)
    kw = dict(restriction=1, interp_type=100)
    dev = mi.BoomerAMG(print_level=0, **kw)
    A = device_matrix(mi, M)
    dev.setup(A)
    _assert_hierarchies_have_the_same_bits(dev, host_amg(mi, ij_host(mi, M), **kw))
    sizes = [dev.level_csr(l, 0)[3][0] for l in range(dev.num_levels)]
    kinds = [dev.restriction_info(l)["kind"] for l in range(dev.num_levels - 1)]
    assert kinds == [1 if n >= 500 else 2 for n in sizes[:-1]] and kinds[:3] == [1, 1, 2], (sizes, kinds)


def test_a_level_with_a_65_point_neighbourhood_says_host(mi, monkeypatch):
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    monkeypatch.setenv("MI_HYPRE_LOCALITY_ORDER", "0")
    M, h = ac.fallback_operator()
    kw = dict(restriction=1, interp_type=100, strong_threshold=0.25)
    dev = mi.BoomerAMG(print_level=0, **kw)
    A = device_matrix(mi, M)
    dev.setup(A)
    _assert_hierarchies_have_the_same_bits(dev, host_amg(mi, ij_host(mi, M), **kw))
    info = dev.restriction_info(0)
    assert info["kind"] == 2 and info["max_m"] == ac.FALLBACK_LENGTH
    kinds = [dev.restriction_info(l)["kind"] for l in range(dev.num_levels - 1)]
    assert 1 in kinds, kinds  # the other levels stay on the device where their neighbourhoods fit


def test_the_singular_neighbourhood_fails_the_device_setup_like_the_host_setup(mi, monkeypatch):
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    monkeypatch.setenv("MI_HYPRE_LOCALITY_ORDER", "0")
    M, _ = ac.singular_case()
    A = device_matrix(mi, M)
    amg = mi.BoomerAMG(print_level=0, restriction=1, max_row_sum=1.0, interp_type=100)
    with pytest.raises(mi.HypreError, match=r"restriction 1\) on level 0: row %d has a singular local system" % ac.SINGULAR_ROW):
        amg.setup(A)
    mi.call("HYPRE_ClearAllErrors")


def test_two_level_solver_matches_the_numpy_cycle(mi):
    """Three cycles of the two-level method (restriction 1, one-point P, C/F Jacobi, exact coarse solve) on the upwind
    operator at 8^3, Peclet 1000: the relative residual of the library's iterate, taken in numpy, against the numpy cycle
    restated from the same operators.  Tolerance: 100 times the distance of the float64 restatement from the longdouble
    one over the three cycles, relative to the last residual.  Measured on an
    MI355X: relative residual 1.4921545128759668e-03 against 1.4921545128759673e-03, float64 against
    longdouble 2.9e-14, tolerance 2.9e-12."""
    cycles = 3
    M = ac.upwind_constant(8, 1000)
    n = M.shape[0]
    f = np.random.default_rng(7).standard_normal(n)
    amg = mi.BoomerAMG(print_level=0, restriction=1, interp_type=100, max_levels=2, relax_type=0, relax_order=1,
                       max_iterations=cycles, tolerance=0.0)
    A = device_matrix(mi, M)
    amg.setup(A)
    assert amg.num_levels == 2 and amg.restriction_info(0)["kind"] == 2  # (512 rows: below the device setup's threshold)
    b, x = device_vector(mi, f), device_vector(mi, np.zeros(n))
    amg.solve(A, b, x)
    got = float(np.linalg.norm(f - M @ x.get()) / np.linalg.norm(f))
    perm = amg.level_perm(0)
    ops = (csr(amg, 0, 0), csr(amg, 0, 2), csr(amg, 0, 3), amg.level_cf(0))
    assert abs(ops[0] - M[perm][:, perm]).max() == 0.0
    h64 = ref.residual_history(*ops, f[perm], cycles)
    hld = ref.residual_history(*ops, f[perm], cycles, dtype=np.longdouble)
    measured = float(np.abs(h64[1:] - hld[1:]).max() / hld[cycles])
    tol = 100.0 * measured
    print("relative residual after %d cycles: library %.17e, numpy %.17e; float64 against longdouble %.3e, tolerance %.3e"
          % (cycles, got, hld[cycles], measured, tol))
    assert abs(got - hld[cycles]) <= tol * hld[cycles]


def test_gmres_with_restriction_1_takes_no_more_iterations(mi):
    """GMRES(50) + AMG (one-point P, C/F Jacobi) to 1e-8 on the upwind operator at 12^3, Peclet 1000, x* = 1: both runs
    converge, the true residual is checked in numpy, and restriction 1 takes no more iterations than restriction 0.
    Measured on an MI355X: 12 iterations (7 levels) with restriction 0, 9 (6 levels) with
    restriction 1."""
    M = ac.upwind_constant(12, 1000)
    n = M.shape[0]
    rhs = M @ np.ones(n)
    its = {}
    for r in (0, 1):
        A = device_matrix(mi, M)
        b, x = device_vector(mi, rhs), device_vector(mi, np.zeros(n))
        amg = mi.BoomerAMG(print_level=0, restriction=r, interp_type=100, relax_type=0, relax_order=1)
        gm = mi.GMRES(tolerance=1e-8, max_iterations=100, kspace=50, print_level=0)
        gm.set_precond(amg)
        gm.setup(A, b, x)
        assert gm.solve(A, b, x) == 0
        true = float(np.linalg.norm(rhs - M @ x.get()) / np.linalg.norm(rhs))
        its[r] = gm.num_iterations
        print("restriction %d: %d iterations, %d levels, true relative residual %.3e" % (r, its[r], amg.num_levels, true))
        assert gm.final_rel_res < 1e-8 and true < 1e-8 and np.abs(x.get() - 1.0).max() < 1e-6
    assert its[1] <= its[0], its


def test_driver_takes_the_keys(tmp_path):
    from tests.test_gpu_app import _run

    text = open(os.path.join(ROOT, "hypre-mini-app_amd", "etc", "laplace_3d.yaml")).read()
    text = re.sub(r"(n[xyz]): 64", r"\1: 16", text)
    text = text.replace("  relax_type: 8\n", "  relax_type: 8\n  interp_type: 100\n  mi_restriction: 1\n"
                        "  mi_strong_threshold_r: 0.25\n  mi_filter_threshold_r: 0.0\n")
    assert "mi_restriction: 1" in text
    out = _run(tmp_path, text)
    assert "not implemented" not in out, out[-2000:]
    assert re.search(r"Setup \d+ : restriction AIR \(approximate ideal restriction\), level 0 built by the", out), out[-2000:]
    m = re.search(r"max \|x - 1\| = ([0-9.eE+-]+)", out)
    assert m and float(m.group(1)) < 1e-6, out[-2000:]


def test_setup_reuse_rebuilds_with_reason_4(mi):
    A = mi.build_laplace_system(8, 8, 8, 7)[0]
    amg = mi.BoomerAMG(print_level=0, restriction=1, setup_reuse=1)
    amg.setup(A)
    assert amg.setup_kind() == (1, 1)
    amg.setup(A)
    assert amg.setup_kind() == (1, 4)
