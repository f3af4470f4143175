"""CPU: the distance-1 approximate ideal restriction (HYPRE_BoomerAMGSetRestriction 1) and the one-point interpolation
(interp_type 100) built by the host routines and the host-only setup, against the numpy
restatement of their specification (tests/air_ref.py): patterns exactly, values to a measured tolerance, their
properties, the singular neighbourhood, every refused setting, whole hierarchies, setup reuse, and the two-grid factor
of the library's own operators with restriction 1 beside restriction 0."""
import os
import re

import numpy as np
import pytest

from tests import air_cases as ac
from tests import air_ref as ref
from tests import mm_interp_ref
from tests.agg2s_common import ROOT, csr, host_amg, ij_host
from tests.mm_interp_common import THETA


@pytest.fixture(scope="module")
def cases():
    """name -> (A, cf, theta_R, phi, float64 restatement, longdouble values), computed once and left unchanged"""
    out = {}
    for name, (A, cf, th, phi) in ac.host_cases().items():
        R64 = ref.air_restriction(A, cf, th, phi)
        Rld, exact = ref.air_restriction(A, cf, th, phi, longdouble=True)
        assert np.array_equal(R64.indptr, Rld.indptr) and np.array_equal(R64.indices, Rld.indices)
        out[name] = (A, cf, th, phi, R64, exact)
    return out


@pytest.fixture(scope="module")
def fallback_level0(mi_lib):
    """Level 0 of the host-only setup on ac.fallback_operator() -- the library's own splitting, with one 65-point
    neighbourhood -- in natural numbering, and the restatements on its A and marker: (hub, M, A, cf, R, R64, exact)"""
    M, h = ac.fallback_operator()
    amg = host_amg(mi_lib, ij_host(mi_lib, M), restriction=1, interp_type=100, strong_threshold=0.25)
    assert amg.restriction_info(0)["max_m"] == ac.FALLBACK_LENGTH
    A, cf, _, R = ac.natural_operators(amg, 0)
    R64 = ref.air_restriction(A, cf, 0.25, 0.0)
    _, exact = ref.air_restriction(A, cf, 0.25, 0.0, longdouble=True)
    return h, M, A, cf, R, R64, exact


@pytest.fixture(scope="module")
def tolerance(cases, fallback_level0):
    """100 times the largest distance of the float64 restatement from the longdouble one over the cases -- the 65-point
    hub operator and level 0 of the fallback operator among them -- (the library eliminates in another order than
    LAPACK): measured 1.35e-16, so 1.35e-14"""
    measured = max([ac.row_relative_deviation(c[4], c[5]) for c in cases.values()]
                   + [ac.row_relative_deviation(fallback_level0[5], fallback_level0[6])])
    print("float64 against longdouble restatement: %.3e; tolerance %.3e" % (measured, 100 * measured))
    assert 0.0 < measured < 1e-14
    return 100.0 * measured


def test_symbols_are_declared_and_exported(mi_lib):
    def text(name):
        return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    for sym in ("HYPRE_BoomerAMGSetRestriction", "HYPRE_BoomerAMGSetStrongThresholdR", "HYPRE_BoomerAMGSetFilterThresholdR"):
        assert re.search(r"HYPRE_Int\s+%s\s*\(" % sym, text("HYPRE_parcsr_ls.h")), sym
        assert hasattr(mi_lib.lib(), sym), sym
    for sym in ("HYPRE_MI_BoomerAMGGetRestrictionInfo", "HYPRE_MI_AIRRestrictionOp", "HYPRE_MI_OnePointInterpOp"):
        assert re.search(r"HYPRE_Int\s+%s\s*\(" % sym, text("HYPRE_mi_ext.h")), sym
        assert hasattr(mi_lib.lib(), sym), sym
    for name in ("air_restriction_op", "one_point_interp_op"):
        assert hasattr(mi_lib, name)
    assert hasattr(mi_lib.BoomerAMG, "restriction_info")


def test_the_cases_hold_what_they_are_for(cases):
    A, cf, hubs = ac.hub_case(ac.GROUP_LENGTHS, 3)
    N = dict(zip(np.flatnonzero(cf == 1), ref.neighbourhoods(A, cf, 0.25)))
    assert [len(N[h]) for h in hubs] == list(ac.GROUP_LENGTHS)
    lens = np.array([len(v) for v in N.values()])
    assert lens.max() == 64 and (lens == 0).sum() >= 2  # (the hub of length 0 and the row that holds its diagonal alone)
    # row counts: not a multiple of a workgroup's rows -- 256 for the per-row kernels, 4 for the 16-lane solve
    assert len(lens) % 256 != 0 and len(lens) > 256 and (lens <= 16).sum() % 4 != 0
    assert ((lens > 16) & (lens <= 32)).sum() >= 2 and (lens > 32).sum() >= 2
    A, cf, th = cases["hubs65"][:3]
    assert sorted(len(v) for v in ref.neighbourhoods(A, cf, th))[-2:] == [64, 65]
    A, cf = ac.filter_case()
    assert int((cf == 1).sum()) == 3  # less than one workgroup of any kernel
    for pe, m in ((1000, 3), (0.6, 6)):  # the prototype's "at most 6 points"
        A, cf, th = cases["upwind8_pe%g" % pe][:3]
        assert max(len(v) for v in ref.neighbourhoods(A, cf, th)) == m
    # the filter: rows that lose some, none and all but the largest entry
    R0, R5 = cases["filter_phi0"][4], cases["filter_phi0.5"][4]
    assert list(np.diff(R0.indptr)) == [4, 3, 5] and list(np.diff(R5.indptr)) == [3, 3, 2]


@pytest.mark.parametrize("name", list(ac.host_cases()))
def test_host_routine_equals_the_restatement(mi_lib, cases, tolerance, name):
    A, cf, th, phi, R64, exact = cases[name]
    R, info = mi_lib.air_restriction_op(A, cf, th, phi, host=True)
    R = ac.as_csr(R)
    assert R.shape == R64.shape
    assert np.array_equal(R.indptr, R64.indptr) and np.array_equal(R.indices, R64.indices), "patterns differ"
    dev = ac.row_relative_deviation(R, exact)
    print("%s: library against longdouble %.3e (tolerance %.3e)" % (name, dev, tolerance))
    assert dev <= tolerance
    N = ref.neighbourhoods(A, cf, th)
    assert info["status"] == 0 and info["bad_row"] == -1
    assert info["max_m"] == max(len(v) for v in N) and info["zero_rows"] == sum(len(v) == 0 for v in N)
    assert info["dropped"] == sum(len(v) for v in N) + len(N) - R.nnz
    assert (info["dropped"] > 0) == (phi > 0)


@pytest.mark.parametrize("name", [k for k, v in ac.host_cases().items() if v[3] == 0.0])
def test_restriction_properties(mi_lib, cases, tolerance, name):
    """R A vanishes on the positions (i, N_i) -- against the size of the terms that cancel there -- and R's C block is the
    identity."""
    A, cf, th, phi, R64, exact = cases[name]
    R = ac.as_csr(mi_lib.air_restriction_op(A, cf, th, phi, host=True)[0])
    cpts = np.flatnonzero(cf == 1)
    RA, scale = (R @ A).tocsr(), (abs(R) @ abs(A)).tocsr()
    worst = 0.0
    for c, N in enumerate(ref.neighbourhoods(A, cf, th)):
        for j in N:
            worst = max(worst, abs(RA[c, j]) / scale[c, j])
    print("%s: largest |(R A)(i, N_i)| against the terms that cancel: %.3e" % (name, worst))
    assert worst <= tolerance
    C = R[:, cpts].tocsr()
    C.eliminate_zeros()
    assert (abs(C - np.eye(len(cpts))) > 0).sum() == 0 and C.nnz == len(cpts)
    # nothing but the neighbourhood and the point itself
    for c, (i, N) in enumerate(zip(cpts, ref.neighbourhoods(A, cf, th))):
        assert set(R.indices[R.indptr[c]:R.indptr[c + 1]]) == set(N) | {i}


def test_one_point_interpolation_tie_and_no_strong_c_point(mi_lib):
    A, strong, cf = ac.one_point_case()
    P = ac.as_csr(mi_lib.one_point_interp_op(A, ac.strong_csr(strong, 6), cf, host=True))
    want = ref.one_point_interp(A, strong, cf)
    assert np.array_equal(P.indptr, want.indptr) and np.array_equal(P.indices, want.indices) and np.array_equal(P.data, want.data)
    assert list(P.indices) == [0, 1, 2, 0, 2] and list(np.diff(P.indptr)) == [1, 1, 1, 1, 1, 0]
    # a special F point (-3) is an F point without a strong C point
    cf3 = cf.copy()
    cf3[5] = -3
    assert ac.same_bits(mi_lib.one_point_interp_op(A, ac.strong_csr(strong, 6), cf3, host=True), (P.indptr, P.indices, P.data, P.shape))


def test_a_singular_neighbourhood_fails_setup_naming_level_and_row(mi_lib):
    mi = mi_lib
    M, gadget = ac.singular_case()
    # the splitting is what the case needs: restriction 0 builds, and the gadget's points are C, F, F, F
    amg = host_amg(mi, ij_host(mi, M), max_row_sum=1.0, interp_type=100)
    cf = ac.natural_marker(amg, 0)
    assert {i: int(cf[i]) for i in gadget} == gadget
    amg = mi.BoomerAMG(print_level=0, restriction=1, max_row_sum=1.0, interp_type=100)
    A = ij_host(mi, M)
    with pytest.raises(mi.HypreError, match=r"restriction 1\) on level 0: row %d has a singular local system" % ac.SINGULAR_ROW):
        mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
    mi.call("HYPRE_ClearAllErrors")
    with pytest.raises(mi.HypreError, match=r"row %d has a singular local system" % ac.SINGULAR_ROW) as e:
        mi.air_restriction_op(M, cf, host=True)
    assert e.value.info["status"] == 2 and e.value.info["bad_row"] == ac.SINGULAR_ROW
    mi.call("HYPRE_ClearAllErrors")


@pytest.mark.parametrize("kw,pattern", [
    (dict(restriction=2), r"restriction 2 is not implemented"),
    (dict(restriction=3), r"restriction 3 is not implemented"),
    (dict(restriction=-1), r"restriction -1 is not implemented"),
    (dict(restriction=1, strong_threshold_r=-0.1), r"strong_threshold_r -0\.1\d* is not implemented"),
    (dict(restriction=1, filter_threshold_r=-0.5), r"filter_threshold_r -0\.5\d* is not implemented"),
    (dict(strong_threshold_r=-0.1), r"strong_threshold_r -0\.1\d* is not implemented"),
    (dict(restriction=0, filter_threshold_r=-0.5), r"filter_threshold_r -0\.5\d* is not implemented"),
    (dict(restriction=1, agg_num_levels=1), r"restriction 1 \(approximate ideal restriction\) with agg_num_levels 1 is not implemented"),
    (dict(interp_type=99), r"interp_type 99 is not implemented \(.*100 one-point"),
    (dict(interp_type=101), r"interp_type 101 is not implemented"),
], ids=lambda v: "-".join("%s%s" % kv for kv in v.items()) if isinstance(v, dict) else None)
def test_each_refused_setting_is_named(mi_lib, kw, pattern):
    mi = mi_lib
    A, _ = mi.build_laplace_system_host(5, 5, 5, 7, 0, 1)
    amg = mi.BoomerAMG(print_level=0, **kw)
    with pytest.raises(mi.HypreError, match=pattern):
        mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
    mi.call("HYPRE_ClearAllErrors")


def test_accepted_settings_and_defaults(mi_lib):
    mi = mi_lib
    A, _ = mi.build_laplace_system_host(6, 6, 6, 7, 0, 1)
    for kw in (dict(restriction=0), dict(restriction=1), dict(restriction=1, strong_threshold_r=0.0),
               dict(restriction=1, filter_threshold_r=0.1), dict(interp_type=100), dict(restriction=0, strong_threshold_r=0.0)):
        amg = host_amg(mi, A, **kw)
        assert amg.num_levels >= 2
        assert amg.restriction_info(0)["kind"] == (2 if kw.get("restriction") else 0)
    # the defaults: theta_R = 0.25, phi = 0
    d, e = host_amg(mi, A, restriction=1), host_amg(mi, A, restriction=1, strong_threshold_r=0.25, filter_threshold_r=0.0)
    assert ac.same_bits(d.level_csr(0, 3), e.level_csr(0, 3))


@pytest.mark.parametrize("interp", [100, 6])
@pytest.mark.parametrize("pe", [1000, 0.6])
def test_hierarchy_levels_equal_the_restatement(mi_lib, tolerance, pe, interp):
    """Every level of the host-only setup at 12^3: R against the restatement on the level's own A and marker, the
    one-point P, the coarse operator R A P; with restriction 0 the same settings still give R = P^T."""
    mi = mi_lib
    M = ac.upwind_constant(12, pe)
    amg = host_amg(mi, ij_host(mi, M), restriction=1, interp_type=interp, filter_threshold_r=0.0)
    assert amg.num_levels >= 3
    for l in range(amg.num_levels - 1):
        A, cf, P, R = ac.natural_operators(amg, l)
        assert set(np.unique(cf)) <= {1, -1}
        R64 = ref.air_restriction(A, cf, 0.25, 0.0)
        _, exact = ref.air_restriction(A, cf, 0.25, 0.0, longdouble=True)
        assert np.array_equal(R.indptr, R64.indptr) and np.array_equal(R.indices, R64.indices), l
        assert ac.row_relative_deviation(R, exact) <= tolerance, l
        info = amg.restriction_info(l)
        N = ref.neighbourhoods(A, cf, 0.25)
        assert info == dict(kind=2, max_m=max(len(v) for v in N), zero_rows=sum(len(v) == 0 for v in N), dropped=0), (l, info)
        if interp == 100:
            want = ref.one_point_interp(A, mm_interp_ref.strength_rows(A, THETA), cf)
            assert np.array_equal(P.indptr, want.indptr) and np.array_equal(P.indices, want.indices)
            assert np.array_equal(P.data, np.ones(P.nnz)) and np.diff(P.indptr).max() == 1  # rows hold a single 1
        Ac = csr(amg, l + 1, 0)
        Al, Pl, Rl = csr(amg, l, 0), csr(amg, l, 2), csr(amg, l, 3)
        assert abs(Ac - (Rl @ Al @ Pl).tocsr()).max() <= 1e-12 * abs(Ac).max(), l
    plain = host_amg(mi, ij_host(mi, M), interp_type=interp)
    for l in range(plain.num_levels - 1):
        assert plain.restriction_info(l) == dict(kind=0, max_m=0, zero_rows=0, dropped=0)
        assert abs(csr(plain, l, 3) - csr(plain, l, 2).T).nnz == 0


def test_the_filter_reaches_the_hierarchy(mi_lib):
    mi = mi_lib
    M = ac.upwind_constant(8, 0.6)
    full = host_amg(mi, ij_host(mi, M), restriction=1, interp_type=100)
    filt = host_amg(mi, ij_host(mi, M), restriction=1, interp_type=100, filter_threshold_r=0.9)
    A, cf, _, R = ac.natural_operators(filt, 0)
    want = ref.air_restriction(A, cf, 0.25, 0.9)
    assert np.array_equal(R.indptr, want.indptr) and np.array_equal(R.indices, want.indices)
    dropped = filt.restriction_info(0)["dropped"]
    assert dropped > 0 and csr(full, 0, 3).nnz - csr(filt, 0, 3).nnz == dropped


def test_a_level_with_a_65_point_neighbourhood(fallback_level0, tolerance):
    """The operator of the GPU test's fallback: the library's own splitting makes the hub a C point with 65 F neighbours,
    and R of that level -- what the device setup takes from the host routine -- is the restatement's: pattern, values,
    and (R A)(i, N_i) = 0."""
    h, M, A, cf, R, R64, exact = fallback_level0
    assert abs(A - M).max() == 0.0
    Ns = ref.neighbourhoods(A, cf, 0.25)
    N = dict(zip(np.flatnonzero(cf == 1), Ns))
    assert cf[h] == 1 and len(N[h]) == ac.FALLBACK_LENGTH and sorted(len(v) for v in N.values())[-2] <= 64
    assert np.array_equal(R.indptr, R64.indptr) and np.array_equal(R.indices, R64.indices)
    print("float64 against longdouble %.3e, library against longdouble %.3e (tolerance %.3e)"
          % (ac.row_relative_deviation(R64, exact), ac.row_relative_deviation(R, exact), tolerance))
    assert ac.row_relative_deviation(R, exact) <= tolerance
    RA, scale = (R @ A).tocsr(), (abs(R) @ abs(A)).tocsr()
    assert max(abs(RA[c, j]) / scale[c, j] for c, Nc in enumerate(Ns) for j in Nc) <= tolerance


def test_setup_reuse_rebuilds_with_reason_4(mi_lib):
    mi = mi_lib
    A, _ = mi.build_laplace_system_host(6, 6, 6, 7, 0, 1)
    for kw in (dict(restriction=1), dict(interp_type=100), dict(restriction=1, interp_type=100)):
        amg = mi.BoomerAMG(print_level=0, setup_reuse=1, **kw)
        mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
        assert amg.setup_kind() == (1, 1)
        mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
        assert amg.setup_kind() == (1, 4), kw
    amg = mi.BoomerAMG(print_level=0, setup_reuse=1)
    mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
    mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
    assert amg.setup_kind() == (2, 0)


@pytest.mark.parametrize("interp", [100, 6])
@pytest.mark.parametrize("n", [8, 12])
def test_two_grid_factor_at_peclet_1000_is_below_the_transpose(mi_lib, n, interp):
    """The stationary residual reduction per cycle over 12 cycles (tests/air_ref.py two_grid_factor: C/F Jacobi as
    relax_type 0, relax_order 1 states it, exact coarse solve) from the library's own level-0 A, P, R and splitting of the
    host-only setup with max_levels 2.  The method's claim: restriction 1 is strictly below restriction 0 for the same P.
    Measured: 8^3 one-point 0.1443 -> 0.0478, ext+i 0.3010 -> 0.0476; 12^3 one-point 0.1956 ->
    0.0890, ext+i 0.3088 -> 0.0717."""
    mi = mi_lib
    M = ac.upwind_constant(n, 1000)
    f = {}
    for r in (0, 1):
        amg = host_amg(mi, ij_host(mi, M), restriction=r, interp_type=interp, max_levels=2, relax_type=0, relax_order=1)
        assert amg.num_levels == 2
        f[r] = ref.two_grid_factor(csr(amg, 0, 0), csr(amg, 0, 2), csr(amg, 0, 3), amg.level_cf(0))
        if r == 0:
            P0 = amg.level_csr(0, 2)
        else:
            assert ac.same_bits(P0, amg.level_csr(0, 2))  # the same P
    print("%d^3, Peclet 1000, interp_type %d: two-grid factor %.4f with R = P^T, %.4f with restriction 1" % (n, interp, f[0], f[1]))
    assert f[1] < f[0]


def test_more_than_one_rank_refuses_restriction_1_and_builds_one_point_interpolation():
    import subprocess
    import sys

    env = dict(os.environ, MI_HYPRE_HOST_THREADS="2", OMP_NUM_THREADS="1", MI_HYPRE_LOCALITY_ORDER="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", "30983", os.path.join(ROOT, "tests", "air_dist_worker.py")]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    assert p.stdout.count("air rank ok") == 2, p.stdout[-4000:]
