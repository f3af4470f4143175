"""GPU: every path through the single-rank level build (BoomerAMG::build_natural) against the
host-only setup of the same matrix, bit for bit -- each interpolation kind, the device splitting and a host splitting
under a device level, both restrictions, every level on the device or only level 0, and the kept stage markers of the
aggressive two-stage levels.  Compared: every level's A, P and R (CSR arrays), the C/F marker, the C-first order, and what
HYPRE_MI_BoomerAMGGetRestrictionInfo / GetInterpCensus report, which also says who built each level."""
import numpy as np
import pytest

from tests.agg2s_common import host_amg

pytestmark = pytest.mark.gpu

# the interpolation kinds of build_natural: settings, aggressive levels, whether sk::interp is asked on a device level
# that is not aggressive (the levels under the aggressive one get the default interp_type 6)
KINDS = {
    "classical6": (dict(interp_type=6), 0, True),
    "direct0": (dict(interp_type=0), 0, True),
    "multipass4": (dict(interp_type=4), 0, False),
    "agg_multipass": (dict(agg_num_levels=1, agg_interp_type=4), 1, True),
    "agg_two_stage5": (dict(agg_num_levels=1, agg_interp_type=5), 1, True),
    "mm16": (dict(interp_type=16), 0, False),
    "mm17": (dict(interp_type=17), 0, False),
    "one_point100": (dict(interp_type=100), 0, False),
}
MATRICES = {"lap7_12": (12, 7), "lap27_8": (8, 27)}
# restriction 1 is refused together with aggressive levels (validate_settings; tests/test_air_spec.py)
# (and the aggressive level of the 27-point operator at 8^3 leaves 8 rows, the coarsest level: one placement there)
CASES = [(m, k, c, r, pl) for m in MATRICES for k in KINDS for c in (8, 6) for r in (0, 1) for pl in ("all_levels", "level0")
         if not (r == 1 and KINDS[k][1]) and not (pl == "level0" and m == "lap27_8" and KINDS[k][1])]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _same_bits(p, q):
    return p[3] == q[3] and np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) and np.array_equal(_bits(p[2]), _bits(q[2]))


@pytest.fixture(scope="module")
def host_hierarchies(mi):
    """the host-only setup of a case, built once and shared by the two placements"""
    built = {}

    def get(matrix, kw):
        key = (matrix,) + tuple(sorted(kw.items()))
        if key not in built:
            n, stencil = MATRICES[matrix]
            Ah = mi.build_laplace_system_host(n, n, n, stencil, 0, 1)[0]
            built[key] = (Ah, host_amg(mi, Ah, **kw))
        return built[key][1]

    return get


@pytest.mark.parametrize("matrix,kind,coarsen,restriction,placement", CASES,
                         ids=["%s-%s-coarsen%d-restriction%d-%s" % c for c in CASES])
def test_device_levels_are_bit_identical_to_the_host_setup(mi, host_hierarchies, matrix, kind, coarsen, restriction, placement,
                                                           monkeypatch):
    settings, nagg, asks_kernel = KINDS[kind]
    kw = dict(settings, coarsen_type=coarsen, restriction=restriction)
    host = host_hierarchies(matrix, kw)
    sizes = [host.level_csr(l, 0)[3][0] for l in range(host.num_levels)]
    assert host.num_levels >= (2 if placement == "all_levels" else 3) and sizes[1] < sizes[0], sizes
    # "level0": the threshold is level 0's row count, so the levels below it are built by the host routines
    threshold = 0 if placement == "all_levels" else sizes[0]
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", str(threshold))
    monkeypatch.setenv("MI_HYPRE_LOCALITY_ORDER", "0")
    n, stencil = MATRICES[matrix]
    A = mi.build_laplace_system(n, n, n, stencil)[0]
    dev = mi.BoomerAMG(print_level=0, keep_agg_markers=1 if nagg else 0, **kw)
    dev.setup(A)

    assert dev.num_levels == host.num_levels
    for l in range(dev.num_levels):
        for which in (0, 2, 3) if l < dev.num_levels - 1 else (0,):
            assert _same_bits(dev.level_csr(l, which), host.level_csr(l, which)), (l, which)
        if l == dev.num_levels - 1:
            break
        assert np.array_equal(dev.level_cf(l), host.level_cf(l)), l
        assert np.array_equal(dev.level_perm(l), host.level_perm(l)), l
        on_device = sizes[l] >= threshold
        assert on_device == (placement == "all_levels" or l == 0), (l, sizes, threshold)
        # who built the level: sk::interp is asked for types 6 and 0 on a device level only (and never declines here);
        # an approximate ideal restriction says 1 = device, 2 = host routine, the transpose of P says 0
        c, hc = dev.interp_census(l), host.interp_census(l)
        asked = asks_kernel and on_device and l >= nagg
        assert c["host"] == (not asked) and not c["fell_back"] and (c["max_bound"] > 0) == asked, (l, c)
        assert hc["host"] and not hc["fell_back"] and hc["max_bound"] == 0, (l, hc)
        r, hr = dev.restriction_info(l), host.restriction_info(l)
        assert r["kind"] == ((1 if on_device else 2) if restriction else 0) and hr["kind"] == (2 if restriction else 0), (l, r, hr)
        assert {k: r[k] for k in ("max_m", "zero_rows", "dropped")} == {k: hr[k] for k in ("max_m", "zero_rows", "dropped")}, l
        if l < nagg and "agg_interp_type" in settings and settings["agg_interp_type"] == 5:
            m1, m2 = dev.level_agg_markers(l)
            h1, h2 = host.level_agg_markers(l)
            assert np.array_equal(m1, h1) and np.array_equal(m2, h2), l
            assert (m2 == 1).sum() < (m1 == 1).sum() < len(m1)
