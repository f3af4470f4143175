"""GPU: the multicolour ordering of the ILU (local_reordering 2 / ilu_reordering_type 2).  The
colouring, perm and the round count against the Python reference (tests/ilu_color_ref.py) exactly; the factors and the
application against the plain path on the matrix P A P^T the test assembles itself, bit for bit; GMRES histories; the
ILU smoother of BoomerAMG; the refusals; poisoned allocations; the driver's sample deck."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from tests import ilu_color_cases as cc
from tests import ilu_color_ref as ref
from tests import ilu_ref
from tests.ilu_color_env_worker import digest, ij

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

# the factor comparisons run where rows are irregular, long, dense, of mixed sign or without their transposed entry, and
# on one stencil
FACTOR_CASES = ("lap27_10", "dense70", "upwind", "ragged", "convdiff")
_IJ = {}


def _mat(mi, name):
    """(IJ matrix of the case, IJ matrix of P A P^T assembled from the reference's perm)"""
    if name not in _IJ:
        M, o = cc.matrix(name), cc.ordering(name)
        _IJ[name] = (ij(mi, M), ij(mi, o.permuted(M)))
    return _IJ[name]


def _check_ordering(got, o, what):
    print(f"{what}: device colours {got['colours']} rounds {got['rounds']} level sets {got['lower_levels']} / "
          f"{got['upper_levels']}; reference colours {o.ncolours} rounds {o.rounds}")
    assert got["reordering"] == 2
    assert np.array_equal(got["colour"], o.colour), what
    assert np.array_equal(got["perm"], o.perm), what
    assert got["colours"] == o.ncolours and got["rounds"] == o.rounds, what


@pytest.mark.parametrize("name", cc.NAMES)
def test_ordering_equals_the_reference(mi, name):
    o = cc.ordering(name)
    ilu = mi.ILU(local_reordering=2)
    ilu.setup(_mat(mi, name)[0])
    got = ilu.ordering()
    _check_ordering(got, o, name)
    # fill 0: a colour class is an independent set, so no factor has more level sets than there are colours
    assert 1 <= got["lower_levels"] <= o.ncolours and 1 <= got["upper_levels"] <= o.ncolours
    ilu.destroy()


def test_without_the_switch_nothing_is_reordered(mi):
    A = _mat(mi, "lap7_16")[0]
    for kw in ({}, dict(local_reordering=0), dict(local_reordering=1)):  # 1 (HYPRE's RCM) stays ignored
        ilu = mi.ILU(**kw)
        ilu.setup(A)
        got = ilu.ordering()
        assert got["reordering"] == 0 and got["colours"] == 0 and got["rounds"] == 0, kw
        assert got["perm"] is None and got["colour"] is None
        # 3 n - 2 level sets per factor of the 7-point operator in its natural order, n = 16
        assert got["lower_levels"] == 46 and got["upper_levels"] == 46
        ilu.destroy()


def _solve(mi, A, ilu, rhs):
    rhs = np.asarray(rhs, dtype=np.float64)
    n = rhs.shape[-1]
    nc = 1 if rhs.ndim == 1 else rhs.shape[0]
    b = mi.IJVector(0, n - 1, rhs.copy(), ncomp=nc)
    x = mi.IJVector(0, n - 1, np.zeros_like(rhs), ncomp=nc)
    ilu.solve(A, b, x)
    return x.get() if nc == 1 else x.get_all()


# (keywords of the setup, relative tolerance of the comparison: 0 = bit for bit).  The asynchronous sweeps (types 1, 2)
# depend on scheduling until they have converged; 200 sweeps are more than the dependency depth of these factors.
CONFIGS = {
    "fill0": (dict(fill=0), 0.0),
    "fill1": (dict(fill=1), 0.0),
    "fill2": (dict(fill=2), 0.0),
    "type3": (dict(iterative_algorithm_type=3, iterative_max_iterations=5), 0.0),
    "type4": (dict(iterative_algorithm_type=4, iterative_max_iterations=5), 0.0),
    "type1": (dict(iterative_algorithm_type=1, iterative_max_iterations=200), 1e-12),
    "type2": (dict(iterative_algorithm_type=2, iterative_max_iterations=200), 1e-12),
}


# ILU(2) of the 27-point operator holds ~300 entries per row and its four serial symbolic passes take 4.5 s: fill 2 runs
# on the other cases
@pytest.mark.parametrize("name,config", [(n, c) for n in FACTOR_CASES for c in CONFIGS if (n, c) != ("lap27_10", "fill2")])
def test_factors_and_application_equal_the_plain_path_on_the_permuted_matrix(mi, name, config):
    kw, rtol = CONFIGS[config]
    o = cc.ordering(name)
    A, B = _mat(mi, name)
    n = o.n
    rng = np.random.default_rng(11)
    rhs = rng.standard_normal((3, n))
    for trisolve in (1, 0):
        mine = mi.ILU(max_iterations=1, tolerance=0.0, trisolve=trisolve, local_reordering=2, **kw)
        plain = mi.ILU(max_iterations=1, tolerance=0.0, trisolve=trisolve, **kw)
        mine.setup(A)
        plain.setup(B)
        assert np.array_equal(mine.ordering()["perm"], o.perm)
        (ia, ja, a), (ia0, ja0, a0) = mine.factors(), plain.factors()
        assert np.array_equal(ia, ia0) and np.array_equal(ja, ja0)
        for b in (rhs[0], rhs):  # one vector, and a multivector of 3 components
            x = _solve(mi, A, mine, b)
            x0 = _solve(mi, B, plain, b[..., o.perm])
            back = np.empty_like(x0)
            back[..., o.perm] = x0
            dev_a, dev_x = np.abs(a - a0).max(), np.abs(x - back).max()
            print(f"{name} {config} trisolve {trisolve} ncomp {b.ndim == 2 and 3 or 1}: max|a - a0| {dev_a:.3e}, "
                  f"max|x - x0| {dev_x:.3e}")
            if rtol == 0.0:
                assert np.array_equal(a, a0) and np.array_equal(x, back), (name, config, trisolve)
            else:
                assert dev_a <= rtol * np.abs(a0).max() and dev_x <= rtol * np.abs(back).max(), (name, config, trisolve)
        mine.destroy()
        plain.destroy()


def test_gmres_history_equals_the_plain_path_on_the_permuted_system(mi):
    name = "lap7_16"
    M, o = cc.matrix(name), cc.ordering(name)
    A, B = _mat(mi, name)
    n = o.n
    f = M @ np.ones(n)
    hist = []
    for mat, rhs, kw in ((A, f, dict(local_reordering=2)), (B, f[o.perm], {})):
        b = mi.IJVector(0, n - 1, rhs.copy())
        x = mi.IJVector(0, n - 1, np.zeros(n))
        gm = mi.GMRES(tolerance=0.0, max_iterations=10, kspace=50, print_level=0)
        ilu = mi.ILU(max_iterations=1, tolerance=0.0, **kw)
        gm.set_precond(ilu)
        gm.setup(mat, b, x)
        gm.solve(mat, b, x)
        hist.append((gm.residual_history(), x.get()))
        gm.destroy()
        ilu.destroy()
    (h, x), (h0, x0) = hist
    print("histories", h, h0, "max relative difference", (np.abs(h - h0) / h0).max())
    assert len(h) == len(h0) == 11
    # per step, the tolerance of the oracle parity tests of tests/test_gpu_amg.py
    assert np.allclose(h, h0, rtol=1e-8, atol=1e-14 * h0[0])
    assert h[-1] < 1e-2 * h[0]  # it preconditions: ten steps take the residual down two orders
    assert np.abs(x[o.perm] - x0).max() <= 1e-8 * np.abs(x0).max()


def _amg_digest(amg, A, x):
    """Setup; the bytes of every level's operator and of every interpolation"""
    x.set(np.zeros(x.get().shape))
    amg.setup(A)
    nl = amg.num_levels
    return [[arr.tobytes() for arr in amg.level_csr(l, w)[:3]] for l in range(nl) for w in (0, 2) if w == 0 or l + 1 < nl]


def _residual(M, f, u, dt):
    """f - M u in dtype dt, every row's sum in stored order"""
    ia, ja, a = M.indptr, M.indices, M.data.astype(dt)
    u = u.astype(dt)
    return f.astype(dt) - np.array([np.dot(a[ia[i]:ia[i + 1]], u[ja[ia[i]:ia[i + 1]]]) for i in range(M.shape[0])], dtype=dt)


def test_ilu_smoother_of_boomeramg(mi):
    A, b, x, rhs = mi.build_laplace_system(12, 12, 12, 7)
    kw = dict(print_level=0, smooth_type=5, smooth_num_levels=2, max_iterations=1, tolerance=0.0)
    amg = mi.BoomerAMG(ilu_reordering_type=2, **kw)
    amg.setup(A)
    assert amg.num_levels >= 3
    rng = np.random.default_rng(5)
    for l in (0, 1):
        ia, ja, a, shape = amg.level_csr(l, 0)
        M = sp.csr_matrix((a, ja, ia), shape=shape)
        o = ref.Ordering(M)
        _check_ordering(amg.level_ilu_ordering(l), o, f"level {l}")
        # one smoother step: u + P^T (LU)^-1 P (f - A u), in longdouble and restated in float64
        n = shape[0]
        f, u = rng.standard_normal(n), rng.standard_normal(n)
        Bm = o.permuted(M)
        want = {}
        for dt in (ilu_ref.LD, np.float64):
            F = ilu_ref.Factors(Bm, 0, dt)
            r = _residual(M, f, u, dt)
            z = np.zeros(n, dtype=dt)
            z[o.perm] = F.apply_exact(r[o.perm])
            want[dt] = u.astype(dt) + z
        got = amg.smooth_level(l, f, u)
        dev, tol = ilu_ref.deviation(got, want[ilu_ref.LD]), ilu_ref.bound(want[np.float64], want[ilu_ref.LD])
        print(f"level {l} smoother step: max|device - longdouble| {dev:.3e}, bound {tol:.3e}")
        assert dev <= tol, (l, dev, tol)
    with pytest.raises(mi.HypreError, match="no ILU smoother"):
        amg.level_ilu_ordering(amg.num_levels - 1)
    mi.call("HYPRE_ClearAllErrors")
    # the value 0 is the library without the key: the same hierarchy and the same cycle, bit for bit
    out = []
    for extra in ({}, dict(ilu_reordering_type=0)):
        amg0 = mi.BoomerAMG(**kw, **extra)
        levels = _amg_digest(amg0, A, x)
        mi.call("HYPRE_BoomerAMGSolve", amg0.h, A.par, b.par, x.par, allow=(mi.HYPRE_ERROR_CONV,))
        assert amg0.level_ilu_ordering(0)["reordering"] == 0
        out.append((levels, x.get().tobytes()))
        amg0.destroy()
    assert out[0] == out[1]
    # and the ordering changes the cycle (the switch reaches the smoothers)
    x.set(np.zeros(x.get().shape))
    mi.call("HYPRE_BoomerAMGSolve", amg.h, A.par, b.par, x.par, allow=(mi.HYPRE_ERROR_CONV,))
    assert x.get().tobytes() != out[0][1] and np.all(np.isfinite(x.get()))


def test_refusals_name_the_callers_row(mi):
    """The matrices of tests/test_gpu_itilu.py::test_refusals -- row 2 stores no diagonal; row 4 stores a_44 = 0 -- and a
    third whose row 3 stores no diagonal, through the exact setup and the iterative types 3 and 1.  The reference puts
    caller row 4 at position 3 and row 3 at position 4 of the reordered block, so the second and third message are
    right only when the row is mapped back; row 4 comes before row 5, so the exact elimination meets the stored zero."""
    missing2 = ([0, 1, 2, 3, 3, 4, 4, 5, 5], [0, 1, 3, 2, 3, 4, 5, 4, 5], [4.0, 4.0, 1.0, 1.0, 4.0, 4.0, 1.0, 1.0, 4.0])
    zero4 = ([0, 1, 2, 2, 3, 3, 4, 4, 5, 5], [0, 1, 2, 3, 2, 3, 4, 5, 4, 5],
             [4.0, 4.0, 4.0, 1.0, 1.0, 4.0, 0.0, 1.0, 1.0, 4.0])
    missing3 = ([0, 1, 2, 2, 3, 4, 4, 5, 5], [0, 1, 2, 3, 2, 4, 5, 4, 5], [4.0, 4.0, 4.0, 1.0, 1.0, 4.0, 1.0, 1.0, 4.0])
    for (rows, cols, vals), bad in ((missing2, 2), (zero4, 4), (missing3, 3)):
        M = sp.csr_matrix((vals, (rows, cols)), shape=(6, 6))
        where = {int(r): q for q, r in enumerate(ref.Ordering(M).perm)}
        if bad != 2:
            assert where[bad] != bad, "the offending row must move for the mapping to show"
        assert where[4] < where[5]
        for typ in (0, 3, 1):
            kw = dict(iterative_algorithm_type=typ, iterative_max_iterations=3) if typ else {}
            ilu = mi.ILU(local_reordering=2, **kw)
            with pytest.raises(mi.HypreError, match=f"row {bad} .*global row {bad}\\)"):
                ilu.setup(ij(mi, M))
            mi.call("HYPRE_ClearAllErrors")
            ilu.destroy()


def test_poisoned_allocations_give_the_same_result(mi):
    """MI_HYPRE_POISON_ALLOC=1 in a fresh process: every device block comes full of 0xFF bytes"""
    names = ["dense70", "ragged"]
    env = dict(os.environ, MI_HYPRE_POISON_ALLOC="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ilu_color_env_worker.py"), *names], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    got = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    assert got == digest(mi, names)
    for name in names:
        assert got[name]["colour"] == cc.ordering(name).colour.tolist()


def test_driver_runs_the_sample_deck(tmp_path):
    from tests.test_gpu_app import _run

    text = open(os.path.join(ROOT, "hypre-mini-app_amd", "etc", "laplace_3d_ilu_multicolor.yaml")).read()
    assert "local_reordering: 2" in text and "preconditioner: ilu" in text
    out = _run(tmp_path, re.sub(r"(n[xyz]): 64", r"\1: 16", text))
    o = cc.ordering("lap7_16")
    assert f"mi_hypre ILU multicolour ordering: {o.ncolours} colours in {o.rounds} rounds" in out, out[-2000:]
    m = re.search(r"mi_hypre ILU\(0\): 4096 rows, \d+ entries, (\d+) lower / (\d+) upper level sets", out)
    assert m and int(m.group(1)) <= o.ncolours and int(m.group(2)) <= o.ncolours, out[-2000:]
    m = re.search(r"max \|x - 1\| = ([0-9.eE+-]+)", out)
    assert m and float(m.group(1)) < 1e-6, out[-2000:]
