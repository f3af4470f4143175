"""GPU: the matrix-matrix extended interpolations (interp_type 16 extended, 17 extended+i) on the
device -- the routine itself through HYPRE_MI_MMInterpOp with every lane count against the numpy restatement
(tests/mm_interp_ref.py), whole hierarchies bit for bit against the host-only setup, repeatability, the zero
denominator, GMRES + AMG beside type 6, the driver."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from tests import mm_interp_cases as mc
from tests import mm_interp_ref as ref
from tests.agg2s_common import host_amg, ij_host, random_mmatrix, zero_denominator_matrix
from tests.mm_interp_common import as_csr, same_pattern_close_values, strength_csr, upwind_convection

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _same_bits(p, q):
    return p[3] == q[3] and np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) and np.array_equal(_bits(p[2]), _bits(q[2]))


@pytest.fixture(scope="module")
def kernel_cases():
    """(A, strong rows, S, marker) of the two kernel cases and their restatements, computed once"""
    out = {}
    for name, make in (("ragged", mc.ragged), ("crafted", mc.crafted)):
        A, strong, S, m = make()
        want = {(t, tf, pmax): ref.mm_interp(A, strong, m, t, tf, pmax) for t in (16, 17) for tf, pmax in ((0.0, 0), (0.2, 4))}
        out[name] = (A, strong, S, m, want)
    return out


def test_the_cases_hold_what_they_are_for(kernel_cases):
    A, strong, S, m, _ = kernel_cases["crafted"]
    assert A.shape[0] <= 200
    c = mc.census(A, strong, m)
    print(c)
    for G in mc.LANES:
        assert c["strong%d" % G] >= 1 and c["strong%d" % (G + 1)] >= 1, G
    for key in ("first", "last", "absent", "beta_zero", "delta_zero", "f_no_strong", "f_only_c"):
        assert c[key] >= 1, key
    A, strong, S, m, _ = kernel_cases["ragged"]
    lens = np.diff(A.indptr)
    assert A.shape[0] == 2000 and lens.min() == 1 and 295 <= lens.max() <= 310 and np.sort(lens)[-2] <= 32
    c = mc.census(A, strong, m)
    assert min(c["first"], c["last"], c["middle"], c["absent"], c["beta_zero"]) > 100


@pytest.mark.parametrize("tf,pmax", [(0.0, 0), (0.2, 4)])
@pytest.mark.parametrize("t", [16, 17])
@pytest.mark.parametrize("name", ["ragged", "crafted"])
def test_kernel_equals_the_restatement_with_every_lane_count(mi, kernel_cases, name, t, tf, pmax):
    A, strong, S, m, want = kernel_cases[name]
    got = {lanes: mi.mm_interp_op(t, A, S, m, tf, pmax, lanes) for lanes in (0,) + mc.LANES}
    same_pattern_close_values(as_csr(got[0]), want[t, tf, pmax])
    for lanes in mc.LANES:
        assert _same_bits(got[lanes], got[0]), lanes


@pytest.mark.parametrize("t", [16, 17])
def test_all_c_all_f_and_the_smallest_sizes(mi, t):
    M = upwind_convection(5)
    n = M.shape[0]
    strong, S = strength_csr(M)
    for lanes in (0, 1, 64):
        ia, ja, a, shape = mi.mm_interp_op(t, M, S, np.ones(n, dtype=np.int32), lanes=lanes)
        assert shape == (n, n) and np.array_equal(ia, np.arange(n + 1)) and np.array_equal(ja, np.arange(n))
        assert np.array_equal(a, np.ones(n))
        for mark in (-1, -3):
            ia, ja, a, shape = mi.mm_interp_op(t, M, S, np.full(n, mark, dtype=np.int32), lanes=lanes)
            assert shape == (n, 0) and np.array_equal(ia, np.zeros(n + 1)) and len(ja) == 0 and len(a) == 0
    E = sp.csr_matrix((0, 0))
    ia, ja, a, shape = mi.mm_interp_op(t, E, E, np.zeros(0, dtype=np.int32))
    assert shape == (0, 0) and np.array_equal(ia, [0]) and len(ja) == 0
    one = sp.csr_matrix(np.array([[2.0]]))
    none = sp.csr_matrix((1, 1))
    ia, ja, a, shape = mi.mm_interp_op(t, one, none, np.array([1], dtype=np.int32))
    assert shape == (1, 1) and np.array_equal(ia, [0, 1]) and np.array_equal(ja, [0]) and np.array_equal(a, [1.0])
    for mark in (-1, -3):
        ia, ja, a, shape = mi.mm_interp_op(t, one, none, np.array([mark], dtype=np.int32))
        assert shape == (1, 0) and np.array_equal(ia, [0, 0])


def test_the_op_refuses_bad_arguments(mi):
    one = sp.csr_matrix(np.array([[2.0]]))
    none = sp.csr_matrix((1, 1))
    for t, cf, lanes in ((18, [1], 0), (17, [0], 0), (17, [1], 3), (17, [1], 128)):
        with pytest.raises(mi.HypreError, match="MMInterpOp"):
            mi.mm_interp_op(t, one, none, np.array(cf, dtype=np.int32), lanes=lanes)
        mi.call("HYPRE_ClearAllErrors")


def _pair(mi, name):
    """the same operator assembled for the device setup and for the host-only setup"""
    if name == "randmm":
        M = random_mmatrix()
        A = mi.IJMatrix(0, M.shape[0] - 1)
        coo = M.tocoo()
        A.set_values_coo(coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data.astype(np.float64))
        A.assemble()
        return A, ij_host(mi, M)
    n, stencil = {"lap7_24": (24, 7), "lap27_16": (16, 27)}[name]
    return mi.build_laplace_system(n, n, n, stencil)[0], mi.build_laplace_system_host(n, n, n, stencil, 0, 1)[0]


def _assert_bit_identical(dev, host, device_built=True):
    assert dev.num_levels == host.num_levels and dev.num_levels > 2
    for l in range(dev.num_levels):
        for which in (0, 2, 3) if l < dev.num_levels - 1 else (0,):
            assert _same_bits(dev.level_csr(l, which), host.level_csr(l, which)), (l, which)
        if l < dev.num_levels - 1:
            assert np.array_equal(dev.level_cf(l), host.level_cf(l)), l
            assert np.array_equal(dev.level_perm(l), host.level_perm(l)), l
            # "another interpolation type": sk::interp was not asked, and nothing fell back to a host routine
            c = dev.interp_census(l)
            assert c["host"] and not c["fell_back"] and c["max_bound"] == 0, (l, c)


@pytest.mark.parametrize("kw", [dict(true_pmax_elmts=4), dict(true_pmax_elmts=0), dict(true_pmax_elmts=4, trunc_factor=0.2)],
                         ids=lambda kw: "-".join("%s%s" % (k.replace("true_", ""), v) for k, v in kw.items()))
@pytest.mark.parametrize("t", [16, 17])
@pytest.mark.parametrize("name", ["lap7_24", "lap27_16", "randmm"])
def test_device_levels_are_bit_identical_to_the_host_setup(mi, name, t, kw, monkeypatch):
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    monkeypatch.setenv("MI_HYPRE_LOCALITY_ORDER", "0")
    A, Ah = _pair(mi, name)
    dev = mi.BoomerAMG(print_level=0, interp_type=t, **kw)
    dev.setup(A)
    _assert_bit_identical(dev, host_amg(mi, Ah, interp_type=t, **kw))


def test_device_levels_with_the_locality_numbering(mi, monkeypatch):
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    monkeypatch.setenv("MI_HYPRE_LOCALITY_ORDER", "1")
    A, Ah = _pair(mi, "lap7_24")
    kw = dict(interp_type=17, true_pmax_elmts=4)
    dev = mi.BoomerAMG(print_level=0, **kw)
    dev.setup(A)
    host = host_amg(mi, Ah, **kw)
    (applied, order), (happlied, horder) = dev.input_ordering(), host.input_ordering()
    assert applied and happlied and np.array_equal(order, horder)
    _assert_bit_identical(dev, host)


def test_other_coarsenings_keep_the_host_splitting_and_use_the_device_interpolation(mi, monkeypatch):
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    monkeypatch.setenv("MI_HYPRE_LOCALITY_ORDER", "0")
    A, Ah = _pair(mi, "lap7_24")
    kw = dict(interp_type=17, coarsen_type=10, true_pmax_elmts=4)
    dev = mi.BoomerAMG(print_level=0, **kw)
    dev.setup(A)
    _assert_bit_identical(dev, host_amg(mi, Ah, **kw))


def test_two_device_setups_are_bit_identical(mi, monkeypatch):
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    monkeypatch.setenv("MI_HYPRE_LOCALITY_ORDER", "0")
    A, _ = _pair(mi, "lap27_16")
    kw = dict(print_level=0, interp_type=17, true_pmax_elmts=4)
    a1, a2 = mi.BoomerAMG(**kw), mi.BoomerAMG(**kw)
    a1.setup(A)
    a2.setup(A)
    _assert_bit_identical(a1, a2)


def test_nothing_reads_memory_it_has_not_written():
    """MI_HYPRE_POISON_ALLOC=1 hands out every device block full of 0xFF bytes: the hierarchies of both types built on
    the device with both truncations (tests/mm_interp_env_worker.py) have the same digest as without -- and as the
    host-only setup, which the worker checks itself."""
    def run(**env):
        e = dict(os.environ, MI_HYPRE_DEVICE_SETUP_MIN_ROWS="0", MI_HYPRE_LOCALITY_ORDER="0", **env)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mm_interp_env_worker.py")], env=e,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-3000:]
        return [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]

    assert run(MI_HYPRE_POISON_ALLOC="1") == run()


@pytest.mark.parametrize("t", [16, 17])
def test_zero_denominator_fails_the_device_setup_like_the_host_setup(mi, t, monkeypatch):
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    monkeypatch.setenv("MI_HYPRE_LOCALITY_ORDER", "0")
    M = zero_denominator_matrix()
    n = M.shape[0]
    msgs = []
    A = mi.IJMatrix(0, n - 1)
    coo = M.tocoo()
    A.set_values_coo(coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data.astype(np.float64))
    A.assemble()
    Ah = ij_host(mi, M)
    for setup in (lambda amg: amg.setup(A), lambda amg: mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, Ah.par)):
        amg = mi.BoomerAMG(print_level=0, interp_type=t)
        with pytest.raises(mi.HypreError, match=r"interp_type %d\) on level 0: row \d+ has a zero denominator" % t) as e:
            setup(amg)
        msgs.append(re.search(r"row \d+", str(e.value)).group(0))
        mi.call("HYPRE_ClearAllErrors")
    assert msgs[0] == msgs[1], msgs


@pytest.mark.parametrize("n,stencil", [(32, 7), (16, 27)])
def test_gmres_converges_with_every_type_and_no_count_doubles(mi, n, stencil):
    """GMRES(50) to 1e-8, x* = 1.  The two-grid factors of types 16 and 17 are within 25 % and 1 % of type 6's
    (tests/test_mm_interp_spec.py): twice type 6's count would mean a defect.  A guard, not a target."""
    its = {}
    for t in (6, 16, 17):
        A, b, x, rhs = mi.build_laplace_system(n, n, n, stencil)
        amg = mi.BoomerAMG(print_level=0, interp_type=t, true_pmax_elmts=4)
        gm = mi.GMRES(tolerance=1e-8, max_iterations=100, kspace=50, print_level=0)
        gm.set_precond(amg)
        gm.setup(A, b, x)
        assert gm.solve(A, b, x) == 0
        assert gm.final_rel_res < 1e-8 and np.abs(x.get() - 1.0).max() < 1e-6, (t, gm.final_rel_res)
        its[t] = gm.num_iterations
        print("%d-point %d^3, interp_type %2d: %d iterations, operator complexity %.3f, %d levels"
              % (stencil, n, t, gm.num_iterations, amg.operator_complexity, amg.num_levels))
    assert its[16] <= 2 * its[6] and its[17] <= 2 * its[6], its


def test_driver_runs_the_sample_deck(tmp_path):
    from tests.test_gpu_app import _run

    text = open(os.path.join(ROOT, "hypre-mini-app_amd", "etc", "laplace_3d_mmext.yaml")).read()
    assert "interp_type: 17" in text
    out = _run(tmp_path, re.sub(r"(n[xyz]): 64", r"\1: 20", text))
    assert "not implemented" not in out and "NOT implemented" not in out, out[-2000:]
    m = re.search(r"max \|x - 1\| = ([0-9.eE+-]+)", out)
    assert m and float(m.group(1)) < 1e-6, out[-2000:]
