"""GPU: the multicolour Gauss-Seidel smoother (relax types 40 / 41 / 42) through the C ABI -- the
colouring and the (block, colour) ordering of every level, the hierarchy against the one relax type 8 builds, the sweep
against the numpy restatement (tests/mcgs_ref.py) on every level of every case of tests/mcgs_cases.py, the value formats,
the zero guess, the collapsed tail, setup reuse, solves, the driver and the refusals."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from tests import air_cases as ac
from tests import mcgs_cases as cases
from tests import mcgs_ref as ref
from tests.agg2s_common import csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV_WORKER = os.path.join(ROOT, "tests", "mcgs_env_worker.py")

pytestmark = pytest.mark.gpu

# The sweep against the float64 restatement, relative to max|u|: 8 x the largest deviation of the float64 restatement
# from the longdouble one over every level of every case, type and weight of test_sweep_equals_the_restatement
# -- measured 4.686e-15 (the wide case; the library itself was then at most 3.82e-15 from the longdouble restatement).
# The test prints the gap it finds and fails when it exceeds the constant.
MEASURED_REF_GAP = 4.7e-15
SWEEP_TOL = 8.0 * MEASURED_REF_GAP  # 3.76e-14
ALL = dict(down_relax_type=40, up_relax_type=41, coarse_relax_type=42)  # every level is coloured and smoothed
CYCLE = dict(down_relax_type=40, up_relax_type=41, coarse_relax_type=9)
_cache = {}


def device_matrix(mi, M):
    A = mi.IJMatrix(0, M.shape[0] - 1)
    coo = sp.coo_matrix(M)
    A.set_values_coo(coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data.astype(np.float64))
    A.assemble()
    return A


def device_vector(mi, v):
    return mi.IJVector(0, len(v) - 1, np.ascontiguousarray(v, dtype=np.float64))


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def hierarchy(mi, name, min_rows, **kw):
    """(operator, IJ matrix, hierarchy with relax types 40 / 41 / 42) of a case; min_rows: the level size from which
    the device builds a level (0: every level; None: the default, so the host routines build these small ones and
    only the colouring and the sort run on the device)"""
    key = (name, min_rows, tuple(sorted(kw.items())))
    if key not in _cache:
        old = os.environ.get("MI_HYPRE_DEVICE_SETUP_MIN_ROWS")
        if min_rows is not None:
            os.environ["MI_HYPRE_DEVICE_SETUP_MIN_ROWS"] = str(min_rows)
        try:
            M = cases.case(name)
            A = device_matrix(mi, M)
            s = dict(ALL)
            s.update(cases.settings(name))
            s.update(kw)
            amg = mi.BoomerAMG(print_level=0, **s)
            amg.setup(A)
            _cache[key] = (M, A, amg)
        finally:
            if min_rows is not None:
                if old is None:
                    del os.environ["MI_HYPRE_DEVICE_SETUP_MIN_ROWS"]
                else:
                    os.environ["MI_HYPRE_DEVICE_SETUP_MIN_ROWS"] = old
    return _cache[key]


def _nc(amg, level):
    return int((amg.level_cf(level) == 1).sum())


STRUCTURE = [(n, 0) for n in cases.CASES] + [("mixed700", None), ("constant_stencil", None), ("many_values", 500),
                                             ("long_row", None), ("diagonal", None)]


@pytest.mark.parametrize("name,min_rows", STRUCTURE)
def test_colours_and_ordering_of_every_level(mi, name, min_rows):
    M, A, amg = hierarchy(mi, name, min_rows)
    nlev = amg.num_levels
    perm0 = amg.level_perm(0).astype(np.int64)
    assert abs(csr(amg, 0, 0) - sp.csr_matrix(M)[perm0][:, perm0]).max() == 0.0  # level 0 is the caller's operator, reordered
    for l in range(nlev):
        B = csr(amg, l, 0)
        n = B.shape[0]
        info, colour = amg.level_colours(l)
        cf, nc = amg.level_cf(l), _nc(amg, l)
        if l < nlev - 1:
            assert np.all(cf[:nc] == 1) and np.all(cf[nc:] != 1), l  # C block first
        assert not ref.colouring_conflicts(B, colour), (l, ref.colouring_conflicts(B, colour)[:4])
        assert np.all(np.diff(colour[:nc]) >= 0) and np.all(np.diff(colour[nc:]) >= 0), l
        assert colour.min() == 0 and info[0] == colour.max() + 1 == len(np.unique(colour)), (l, info)
        assert info[0] <= ref.max_degree(B) + 1, (l, info)
        assert 1 <= info[1] <= n and (info[2], info[3]) == ref.colour_ranges(colour, nc), (l, info)
        # stable: inside a (block, colour) range the rows keep the order they have in the level's own numbering
        perm = amg.level_perm(l).astype(np.int64)
        if n > 1:
            assert sorted(perm.tolist()) == list(range(n))
            same = np.diff(colour) == 0
            if 0 < nc < n:
                same[nc - 1] = False  # (the last C row and the first F row are not one range)
            assert np.all(np.diff(perm)[same] > 0), l
        print("%s level %d: n %d, nc %d, %d colours in %d rounds, %d + %d ranges" % ((name, l, n, nc) + info))
    if name == "diagonal":
        assert nlev == 1 and amg.level_colours(0)[0][0] == 1 and amg.level_colours(0)[0][2:] == (0, 1)
    if name == "wide":
        assert amg.level_colours(0)[0][0] > 30 and np.bincount(amg.level_colours(0)[1]).min() == 1  # ranges of one row


@pytest.mark.parametrize("name,min_rows,kw", [("mixed700", 0, {}), ("upwind", 0, {}), ("constant_stencil", 0, {}),
                                              ("lap27_6", None, {}), ("many_values", 500, {}),
                                              ("constant_stencil", 0, dict(agg_num_levels=1, agg_interp_type=5)),
                                              ("mixed700", 0, dict(num_functions=2))])
def test_hierarchy_is_the_one_relax_type_8_builds(mi, name, min_rows, kw):
    """A, cf, P and R of every level in natural numbering: bit for bit those of the same settings with relax type 8"""
    M, A, amg = hierarchy(mi, name, min_rows, **kw)
    plain = hierarchy(mi, name, min_rows, down_relax_type=8, up_relax_type=8, coarse_relax_type=8, **kw)[2]
    assert amg.num_levels == plain.num_levels
    for l in range(amg.num_levels - 1):
        for got, want in zip(ac.natural_operators(amg, l), ac.natural_operators(plain, l)):
            if sp.issparse(got):
                assert got.shape == want.shape and np.array_equal(got.indptr, want.indptr), l
                assert np.array_equal(got.indices, want.indices) and np.array_equal(bits(got.data), bits(want.data)), l
            else:
                assert np.array_equal(got, want), l
    if kw.get("num_functions"):
        for l in range(amg.num_levels):  # dof_func follows the rows
            p, q = amg.level_perm(l).astype(np.int64), plain.level_perm(l).astype(np.int64)
            a, b = np.empty(len(p), dtype=np.int64), np.empty(len(q), dtype=np.int64)
            a[p], b[q] = amg.level_dof_func(l), plain.level_dof_func(l)
            assert np.array_equal(a, b), l


SWEEPS = [(n, 0) for n in cases.CASES] + [("mixed700", None), ("constant_stencil", None), ("wide", None)]


@pytest.mark.parametrize("name,min_rows", SWEEPS)
def test_sweep_equals_the_restatement(mi, name, min_rows):
    """relax_level(level, 40 / 41 / 42, 0) with weight 1 and 0.8 on every level against sequential substitution on
    level_csr(level, 0); the same sweep twice gives the same bits, its zero-guess route those of an explicit zero vector,
    and the result is not a Jacobi step's (a kernel that read a snapshot of u would give exactly that)."""
    M, A, amg = hierarchy(mi, name, min_rows)
    rng = np.random.default_rng(11)
    gap = worst = 0.0
    try:
        for l in range(amg.num_levels):
            B = csr(amg, l, 0)
            n = B.shape[0]
            f, u = rng.standard_normal(n), rng.standard_normal(n)
            coupled = B.nnz > n
            for omega in (1.0, 0.8):
                mi.call("HYPRE_BoomerAMGSetRelaxWt", amg.h, omega)
                for t in (40, 41, 42):
                    got = amg.relax_level(l, t, 0, f, u)
                    assert np.array_equal(bits(got), bits(amg.relax_level(l, t, 0, f, u))), (l, t)
                    want = ref.sweep(B, u, f, omega, t)
                    wide = ref.sweep(B, u, f, omega, t, dtype=np.longdouble)
                    scale = float(np.abs(wide).max())
                    gap = max(gap, float(np.abs(want - wide).max()) / scale)
                    err = float(np.abs(got - wide).max()) / scale
                    worst = max(worst, err)
                    assert err <= SWEEP_TOL, (l, t, omega, err, SWEEP_TOL)
                    if coupled:
                        jac = amg.relax_level(l, 0, 0, f, u)
                        assert np.abs(got - jac).max() > 1e-3 * np.abs(got).max(), (l, t)
                        assert np.abs(jac - ref.jacobi(B, u, f, omega)).max() <= 1e-12 * np.abs(jac).max()
                zero = amg.relax_pair_level(l, 42, 1, f)  # u None: relax(.., u_is_zero)
                assert np.array_equal(bits(zero), bits(amg.relax_level(l, 42, 0, f, np.zeros(n)))), l
    finally:
        mi.call("HYPRE_BoomerAMGSetRelaxWt", amg.h, 1.0)
        print("%s: float64 restatement against longdouble %.3e, library against longdouble %.3e (of max|u|)" % (name, gap, worst))
    assert gap <= MEASURED_REF_GAP, (gap, MEASURED_REF_GAP)


def test_value_storage_modes_give_the_same_bits(mi):
    """levels >= 1 with fp32 value storage: mode 1 (floats) and mode 2 (fp64 holding the rounded values) run their own
    instantiations of the in-place pass and give the same bits"""
    M = cases.case("constant_stencil")
    A = device_matrix(mi, M)
    amgs = {m: mi.BoomerAMG(print_level=0, mi_value_storage=m, **ALL) for m in (1, 2)}
    for a in amgs.values():
        a.setup(A)
    rng = np.random.default_rng(5)
    kinds = set()
    for l in range(1, amgs[1].num_levels):
        n = amgs[1].level_csr(l, 0)[3][0]
        f, u = rng.standard_normal(n), rng.standard_normal(n)
        kinds.add((amgs[1].level_value_storage(l, 0)[0], amgs[2].level_value_storage(l, 0)[0]))
        for t in (40, 41, 42):
            mi.profile_enable(mi.PROF_LVL_RELAX_MC + l)
            one = amgs[1].relax_level(l, t, 0, f, u)
            name1 = mi.profile_kernel_name(mi.PROF_LVL_RELAX_MC + l)
            two = amgs[2].relax_level(l, t, 0, f, u)
            name2 = mi.profile_kernel_name(mi.PROF_LVL_RELAX_MC + l)
            assert np.array_equal(bits(one), bits(two)), (l, t)
            assert re.match(r"spmv_stream(_xc)?<3, 0", name1) and re.match(r"spmv_stream(_xc)?<3, 0", name2), (name1, name2)
            if amgs[1].level_value_storage(l, 0)[0] == 1:
                assert name1 != name2 and ("float" in name1 or "true>" in name1), (name1, name2)
    assert (1, 2) in kinds, kinds


def _child(mode, **env):
    e = dict(os.environ, **{k: str(v) for k, v in env.items()})
    p = subprocess.run([sys.executable, ENV_WORKER, mode], env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    out = json.loads([line for line in p.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    out["stdout"] = p.stdout
    return out


def _unhex(h):
    return np.frombuffer(bytes.fromhex(h), dtype=np.float64)


def test_value_dictionary_on_and_off():
    """MI_HYPRE_VALUE_DICT 0 against 1 (read once per process): level 0 of the constant stencil runs the dictionary
    instantiation or the plain one; the sweeps agree within the tolerance of the sweep test"""
    on, off = _child("dict", MI_HYPRE_VALUE_DICT=1), _child("dict", MI_HYPRE_VALUE_DICT=0)
    assert on["kind"] == 8 and off["kind"] == 0, (on["kind"], off["kind"])
    assert "true, 256>" in on["kernel"] and on["kernel"] != off["kernel"], (on["kernel"], off["kernel"])
    for t in ("40", "41", "42"):
        a, b = _unhex(on[t]), _unhex(off[t])
        assert np.abs(a - b).max() <= SWEEP_TOL * np.abs(a).max(), t


def test_collapsed_tail_tabulates_the_cycle():
    """MI_HYPRE_DENSE_TAIL_ROWS 0 against the default: one cycle (down 40, up 41) agrees to 1e-12 relative"""
    with_tail = _child("tail", MI_HYPRE_SETUP_TIMING=1)
    without = _child("tail", MI_HYPRE_SETUP_TIMING=1, MI_HYPRE_DENSE_TAIL_ROWS=0)
    said = r"collapsed coarse tail: levels \d+\.\. as one"
    assert re.search(said, with_tail["stdout"]) and not re.search(said, without["stdout"])
    assert re.search(r"multicolour ordering: level 0: n 1728, \d+ colours", with_tail["stdout"])
    a, b = _unhex(with_tail["x"]), _unhex(without["x"])
    assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()


def _solve(mi, M, kw, solver="gmres"):
    n = M.shape[0]
    rhs = M @ np.ones(n)
    A = device_matrix(mi, M)
    b, x = device_vector(mi, rhs), device_vector(mi, np.zeros(n))
    amg = mi.BoomerAMG(print_level=0, **kw)
    ks = (mi.GMRES(tolerance=1e-8, max_iterations=100, kspace=50, print_level=0) if solver == "gmres" else
          mi.PCG(tolerance=1e-8, max_iterations=100, print_level=0, two_norm=1))
    ks.set_precond(amg)
    ks.setup(A, b, x)
    rc = ks.solve(A, b, x)
    xs = x.get()
    return rc, ks.num_iterations, float(np.linalg.norm(rhs - M @ xs) / np.linalg.norm(rhs)), xs


def test_zero_guess_cycle_is_the_general_cycle(mi):
    """every cycle of a preconditioned solve starts from a zero guess: with the zero-guess routes switched off
    (HYPRE_MI_SetZeroGuessMode 0: every sweep reads a vector of zeros like any other) the solve gives the same bits"""
    M = cases.laplace(12, 7)
    try:
        mi.call("HYPRE_MI_SetZeroGuessMode", 0)
        general = _solve(mi, M, CYCLE)
    finally:
        mi.call("HYPRE_MI_SetZeroGuessMode", 3)
    routed = _solve(mi, M, CYCLE)
    assert routed[0] == 0 and routed[1] == general[1] and np.array_equal(bits(routed[3]), bits(general[3]))


@pytest.mark.parametrize("name", ["lap7_16", "lap27_16", "upwind12"])
def test_gmres_with_the_multicolour_cycle_converges(mi, name):
    M = {"lap7_16": lambda: cases.laplace(16, 7), "lap27_16": lambda: cases.laplace(16, 27),
         "upwind12": lambda: ac.upwind_constant(12, 30)}[name]()
    its = {}
    for label, kw in (("40/41", CYCLE), ("8", dict(relax_type=8)), ("6", dict(relax_type=6))):
        rc, its[label], true, xs = _solve(mi, M, kw)
        if label == "40/41":
            assert rc == 0 and its[label] <= 100 and true <= 1e-8 * (1.0 + 1e-6), (rc, its, true)
    print("%s: GMRES iterations, one sweep per leg: down 40 / up 41: %d, relax type 8: %d, relax type 6: %d"
          % (name, its["40/41"], its["8"], its["6"]))


def test_pcg_with_the_symmetric_multicolour_cycle_converges(mi):
    M = cases.laplace(16, 7)
    its = {}
    for label, kw in (("40/41", CYCLE), ("8", dict(relax_type=8)), ("6", dict(relax_type=6))):
        rc, its[label], true, xs = _solve(mi, M, kw, solver="pcg")
        if label == "40/41":
            assert rc == 0 and its[label] <= 100 and true <= 1e-8 * (1.0 + 1e-6), (rc, its, true)
    print("lap7_16: PCG iterations: down 40 / up 41: %d, relax type 8: %d, relax type 6: %d" % (its["40/41"], its["8"], its["6"]))


def test_setup_reuse_keeps_colours_and_ordering(mi):
    M0 = cases.case("mixed700")
    M1 = M0.copy()
    M1.data = M0.data * (1.0 + 0.1 * np.random.default_rng(9).random(M0.nnz))
    A = device_matrix(mi, M0)
    amg = mi.BoomerAMG(print_level=0, setup_reuse=1, strong_threshold=0.25, **ALL)
    amg.setup(A)
    assert amg.setup_kind() == (1, 1)
    before = [(amg.level_colours(l), amg.level_perm(l)) for l in range(amg.num_levels)]
    coo = M1.tocoo()
    A.initialize()
    A.set_values_coo(coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data.astype(np.float64))
    A.assemble()
    amg.setup(A)
    assert amg.setup_kind() == (2, 0), amg.setup_kind()
    rng = np.random.default_rng(10)
    for l, ((info, colour), perm) in enumerate(before):
        now = amg.level_colours(l)
        assert now[0] == info and np.array_equal(now[1], colour) and np.array_equal(amg.level_perm(l), perm), l
        B = csr(amg, l, 0)
        n = B.shape[0]
        f, u = rng.standard_normal(n), rng.standard_normal(n)
        got, want = amg.relax_level(l, 42, 0, f, u), ref.sweep(B, u, f, 1.0, 42)
        assert np.abs(got - want).max() <= SWEEP_TOL * np.abs(want).max(), l
    p0 = amg.level_perm(0).astype(np.int64)
    assert abs(csr(amg, 0, 0) - M1[p0][:, p0]).max() == 0.0  # the refreshed operator
    # the presence of 40 / 41 / 42 is structural: without them the next Setup rebuilds (reason 3) and keeps no colours
    mi.call("HYPRE_BoomerAMGSetRelaxType", amg.h, 8)
    amg.setup(A)
    assert amg.setup_kind() == (1, 3)
    with pytest.raises(mi.HypreError, match="was not coloured"):
        amg.level_colours(0)
    mi.call("HYPRE_ClearAllErrors")


def test_relax_type_set_after_setup_needs_a_setup(mi):
    M = cases.laplace(8, 7)
    n = M.shape[0]
    A = device_matrix(mi, M)
    b, x = device_vector(mi, M @ np.ones(n)), device_vector(mi, np.zeros(n))
    amg = mi.BoomerAMG(print_level=0, relax_type=8)
    amg.setup(A)
    amg.solve(A, b, x)
    mi.call("HYPRE_BoomerAMGSetRelaxType", amg.h, 40)
    with pytest.raises(mi.HypreError, match=r"returned 4: .*relax type 40 \(multicolour Gauss-Seidel\).*a Setup is needed"):
        amg.solve(A, b, x)
    mi.call("HYPRE_ClearAllErrors")
    amg.setup(A)  # and the Setup it asks for makes the same handle work
    amg.solve(A, b, x)
    assert amg.level_colours(0)[0][0] >= 2


@pytest.mark.parametrize("kind", ["missing", "zero"])
@pytest.mark.parametrize("min_rows", [0, None])
def test_missing_or_zero_diagonal_names_level_and_row(mi, kind, min_rows, monkeypatch):
    if min_rows is not None:
        monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", str(min_rows))
    M = cases.laplace(6, 7)
    row = 77
    s = slice(M.indptr[row], M.indptr[row + 1])
    M.data[s][M.indices[s] == row] = 0.0  # (a view: the stored a_ii becomes an explicit zero)
    if kind == "missing":
        M.eliminate_zeros()
    assert M[row, row] == 0.0 and (M.nnz == 1296) == (kind == "zero")
    A = device_matrix(mi, M)
    amg = mi.BoomerAMG(print_level=0, **ALL)
    what = "stores no diagonal entry" if kind == "missing" else "stores a zero diagonal entry"
    with pytest.raises(mi.HypreError, match=r"multicolour Gauss-Seidel\): level 0, row %d \(.*\) %s" % (row, what)):
        amg.setup(A)
    mi.call("HYPRE_ClearAllErrors")


def test_driver_runs_the_sample_deck(tmp_path):
    from tests.test_gpu_app import _run

    text = open(os.path.join(ROOT, "hypre-mini-app_amd", "etc", "laplace_3d_multicolor_gs.yaml")).read()
    assert "down_relax_type: 40" in text and "up_relax_type: 41" in text
    text = re.sub(r"(n[xyz]): \d+", r"\1: 8", text)
    out = _run(tmp_path, text)
    assert "not implemented" not in out, out[-2000:]
    m = re.search(r"max \|x - 1\| = ([0-9.eE+-]+)", out)
    assert m and float(m.group(1)) < 1e-6, out[-2000:]
