"""GPU: the batched multivector kernels -- spmv_stream_xc_mv<NV, ...>, gs_tile_mv_k<NV, ...> -- and the batched
BoomerAMG cycle built on them (HYPRE_MI_SetMultivectorBatch).

The contract is one sentence: a batched pass gives, component by component, the bits the component-by-component path
gives.  So every comparison here is an equality of bit patterns (`same`, as in tests/test_gpu_value_dictionary.py)
against the library's own single-vector path, which the other suites hold against the oracle; there is no tolerance.
Which kernel ran is read from the instantiation name a launch leaves in its profile class, how many passes ran batched
from the counters mv_batched_matvecs / mv_batched_cycles / mv_fallback_cycles."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import dict_cases as dc
from tests.systems import convection_diffusion_3d, three_component_rhs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS_TYPES = [3, 4, 6, 8, 13, 14]
RELAX_NAMES = list(dc.RELAX) + [k for k in dc.ZERO if k not in dc.RELAX]


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def first_difference(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64).ravel(), np.ascontiguousarray(b, dtype=np.float64).ravel()
    d = np.flatnonzero(a.view(np.int64) != b.view(np.int64))
    return None if len(d) == 0 else (int(d[0]), float(a[d[0]]), float(b[d[0]]), len(d))


@pytest.fixture
def width(mi):
    """set(width); the width found on entry is put back afterwards"""
    before = mi.multivector_batch()
    try:
        yield mi.set_multivector_batch
    finally:
        mi.set_multivector_batch(before)


@pytest.fixture
def dictionary(mi):
    try:
        yield mi.set_value_dictionary
    finally:
        mi.set_value_dictionary(True)


@pytest.fixture
def kernel_names(mi):
    pids = (mi.PROF_SPMV_L0, mi.PROF_LVL_RELAX, mi.PROF_LVL_RELAX + 1, mi.PROF_LVL_RELAX0, mi.PROF_LVL_RELAX0 + 1)
    for pid in pids:
        mi.profile_enable(pid, 8)
    try:
        yield mi.profile_kernel_name
    finally:
        for pid in pids:
            mi.profile_enable(pid, 0)


@pytest.fixture
def zero_guess_mode(mi):
    try:
        yield lambda mode: mi.call("HYPRE_MI_SetZeroGuessMode", mode)
    finally:
        mi.call("HYPRE_MI_SetZeroGuessMode", 3)


def _vectors(rng, nvec, n):
    """nvec vectors; one of them all zeros and one of magnitude >= 1e150: a component that leaked into another shows"""
    V = rng.standard_normal((nvec, n))
    V[nvec - 1] = 0.0
    V[0] = np.where(V[0] < 0.0, -1.0, 1.0) * (1e150 + 1e150 * np.abs(V[0]))
    return V


def _mv_name(single, nvec):
    """the batched instantiation beside a single-vector one"""
    if single.startswith("gs_tile_k<"):
        return single.replace("gs_tile_k<", "gs_tile_mv_k<%d, " % nvec)
    return single.replace("spmv_stream_xc<0, ", "spmv_stream_xc_mv<%d, " % nvec)


# ---------------------------------------------------------------- 1. SpMV
@pytest.mark.parametrize("name", list(dc.SPMV) + list(dc.GIANT))
def test_spmv(mi, width, dictionary, kernel_names, name):
    M, info = dc.spmv_case(name)
    n = M.shape[0]
    w = 512 if M.nnz / n >= 100.0 else 256
    rng = np.random.default_rng(7 + n)
    for on in (True, False):
        dictionary(on)
        A = mi.matrix_from_scipy(M)
        dictionary(True)
        assert mi.parcsr_value_kind(A) == (info["kind"] if on else 0)
        flag = "true" if (on and info["kind"] == 8) else "false"
        single = ("spmv_stream_xc<0, 0, %s, 512>" if w == 512 else "spmv_stream_xc<0, 1, %s, 256>") % flag
        for nvec in (2, 3, 4, 5):
            X, B = _vectors(rng, nvec, n), _vectors(rng, nvec, n)[::-1].copy()
            for alpha, beta in ((1.0, 0.0), (-1.5, 0.75)):
                ref = np.empty((nvec, n))
                for c in range(nvec):
                    x1, y1 = mi.IJVector(0, n - 1, X[c]), mi.IJVector(0, n - 1, B[c])
                    mi.call("HYPRE_ParCSRMatrixMatvec", alpha, A.par, x1.par, beta, y1.par)
                    ref[c] = y1.get()
                assert kernel_names(mi.PROF_SPMV_L0) == single
                x = mi.IJVector(0, n - 1, X, ncomp=nvec)
                for wd, passes in ((4, (nvec + 3) // 4), (3, (nvec + 2) // 3), (1, 0)):
                    width(wd)
                    y = mi.IJVector(0, n - 1, B, ncomp=nvec)  # y holds b
                    before = mi.counter("mv_batched_matvecs")
                    mi.parcsr_matvec_multi(alpha, A, x, beta, y)
                    assert mi.counter("mv_batched_matvecs") - before == passes, (nvec, wd)
                    got = y.get_all()
                    kname = kernel_names(mi.PROF_SPMV_L0)
                    # the last launch: a batch of the last group's size, or the single-vector kernel on a lone component
                    last = 1 if wd == 1 else (nvec % wd or wd)
                    assert kname == (single if last == 1 else _mv_name(single, last)), (kname, nvec, wd)
                    assert same(got, ref), (name, on, nvec, wd, alpha, beta, kname, first_difference(got, ref))
                assert np.isfinite(ref).all() and np.abs(ref[0]).max() > 1e140 and (beta != 0.0 or not ref[nvec - 1].any())
        A.destroy()


def test_matvec_multi_refusals(mi):
    M, _ = dc.spmv_case("rowlen33")
    n = M.shape[0]
    A = mi.matrix_from_scipy(M)
    x3, y2 = mi.IJVector(0, n - 1, np.zeros((3, n)), ncomp=3), mi.IJVector(0, n - 1, np.zeros((2, n)), ncomp=2)
    for a, b in ((x3, y2), (x3, x3)):
        with pytest.raises(mi.HypreError, match="ParCSRMatrixMatvecMulti"):
            mi.parcsr_matvec_multi(1.0, A, a, 0.0, b)
        mi.call("HYPRE_ClearAllErrors")


# ---------------------------------------------------------------- 2. relaxation
def _amg(mi, M, **kw):
    A = mi.matrix_from_scipy(M)
    amg = mi.BoomerAMG(print_level=0, **kw)
    amg.setup(A)
    return A, amg


def _level_rows(mi, amg, level):
    nr, nc, nnz = mi.c_int(), mi.c_int(), mi.c_big()
    mi.call("HYPRE_MI_BoomerAMGGetLevelCSRSize", amg.h, level, 0, mi.C.byref(nr), mi.C.byref(nc), mi.C.byref(nnz))
    return nr.value


def _check_passes(mi, names, amg, level, rng, types, expect=None):
    """RelaxLevelMulti for points 0 / +1 / -1 and nvec 2, 3, 4 against RelaxLevel on each component.  expect: the
    single-vector instantiation the level must run (None: whatever it runs); returns the names seen."""
    n = _level_rows(mi, amg, level)
    pid = mi.PROF_LVL_RELAX + level
    seen = set()
    for rtype in types:
        F, U = _vectors(rng, 4, n), _vectors(rng, 4, n)[::-1].copy()
        for points in (0, 1, -1):
            ref = np.stack([amg.relax_level(level, rtype, points, F[c], U[c]) for c in range(4)])
            single = names(pid)
            assert expect is None or single == expect, (single, expect)
            for nvec in (2, 3, 4):
                got = amg.relax_level_multi(level, rtype, points, F[:nvec], U[:nvec])
                kname = names(pid)
                seen.add(kname)
                assert kname == _mv_name(single, nvec) if single.startswith("gs_tile_k<") else kname == single, (kname, single)
                assert same(got, ref[:nvec]), (level, rtype, points, nvec, kname, first_difference(got, ref[:nvec]))
    return seen


def _check_pairs(mi, names, amg, level, rng, types):
    """RelaxPairLevelMulti, first +-1 x zero guess or not, against RelaxPairLevel on each component"""
    n = _level_rows(mi, amg, level)
    seen = set()
    for rtype in types:
        F, U = _vectors(rng, 4, n), _vectors(rng, 4, n)[::-1].copy()
        for first in (1, -1):
            for zero in (False, True):
                pid = (mi.PROF_LVL_RELAX0 if zero else mi.PROF_LVL_RELAX) + level
                ref = np.stack([amg.relax_pair_level(level, rtype, first, F[c], None if zero else U[c]) for c in range(4)])
                single = names(pid)
                for nvec in (2, 3, 4):
                    got = amg.relax_pair_level_multi(level, rtype, first, F[:nvec], None if zero else U[:nvec])
                    kname = names(pid)
                    seen.add(kname)
                    assert kname == _mv_name(single, nvec) if single.startswith("gs_tile_k<") else kname == single, (kname, single)
                    assert same(got, ref[:nvec]), (level, rtype, first, zero, nvec, kname, first_difference(got, ref[:nvec]))
    return seen


@pytest.mark.parametrize("on", [True, False], ids=["dictionary", "plain"])
@pytest.mark.parametrize("name", RELAX_NAMES)
def test_relaxation_passes(mi, width, dictionary, kernel_names, name, on):
    """levels 0 and 1 of every relaxation operator, zero-guess mode 3 (the default: pairs run on the sub-operators and
    the F pass leaves `tout`)"""
    width(4)
    M = dc.relax_case(name)
    dictionary(on)
    A, amg = _amg(mi, M)
    dictionary(True)
    assert amg.num_levels > 1 and amg.level_value_storage(0, 0)[0] == (8 if on else 0)
    w = 512 if M.nnz / M.shape[0] >= 100.0 else 256
    rng = np.random.default_rng(31 + M.shape[0])
    seen = _check_passes(mi, kernel_names, amg, 0, rng, GS_TYPES, expect="gs_tile_k<%s, %d>" % ("true" if on else "false", w))
    assert seen == {"gs_tile_mv_k<%d, %s, %d>" % (nv, "true" if on else "false", w) for nv in (2, 3, 4)}
    _check_passes(mi, kernel_names, amg, 1, rng, GS_TYPES)
    for level in (0, 1):
        _check_pairs(mi, kernel_names, amg, level, rng, GS_TYPES)


@pytest.mark.parametrize("on", [True, False], ids=["dictionary", "plain"])
@pytest.mark.parametrize("name", RELAX_NAMES)
def test_zero_guess_pairs_mode_1(mi, width, dictionary, kernel_names, zero_guess_mode, name, on):
    """mode 1: the pairs sweep the level operator itself and are told where the zeros start"""
    width(4)
    zero_guess_mode(1)
    dictionary(on)
    M = dc.relax_case(name)
    w = 512 if M.nnz / M.shape[0] >= 100.0 else 256
    A, amg = _amg(mi, M)
    dictionary(True)
    rng = np.random.default_rng(57 + len(name))
    for level in (0, 1):
        seen = _check_pairs(mi, kernel_names, amg, level, rng, GS_TYPES)
        if level == 0:
            assert seen == {"gs_tile_mv_k<%d, %s, %d>" % (nv, "true" if on else "false", w) for nv in (2, 3, 4)}, seen


def test_relaxation_on_fp32_levels(mi, width, dictionary, kernel_names):
    """HYPRE_MI_BoomerAMGSetValueStorage mode 1: level 1 streams floats (no dictionary: it would win)"""
    width(4)
    M, A1 = dc.pendant_operator("rowlen17")
    dictionary(False)
    A, amg = _amg(mi, M, mi_value_storage=1)
    dictionary(True)
    assert amg.level_value_storage(1, 0)[0] == 1
    rng = np.random.default_rng(77)
    seen = _check_passes(mi, kernel_names, amg, 1, rng, GS_TYPES, expect="gs_tile_k<false, 256, true>")
    assert seen == {"gs_tile_mv_k<%d, false, 256, true>" % nv for nv in (2, 3, 4)}
    _check_pairs(mi, kernel_names, amg, 1, rng, [3, 8, 14])


def test_relaxation_where_the_launcher_loops(mi, width, kernel_names):
    """HYPRE_MI_SetGSChunk(4): gs_hybrid_k has no batched form -- the same hook, the same bits, the single-vector name"""
    width(4)
    mi.call("HYPRE_MI_SetGSChunk", 4)
    try:
        A, amg = _amg(mi, dc.relax_case("rowlen17"))
        rng = np.random.default_rng(5)
        assert _check_passes(mi, kernel_names, amg, 0, rng, [3, 8, 14], expect="gs_hybrid_k") == {"gs_hybrid_k"}
        _check_pairs(mi, kernel_names, amg, 0, rng, [6, 13])
    finally:
        mi.call("HYPRE_MI_SetGSChunk", 8)


def test_relax_multi_refusals(mi):
    A, amg = _amg(mi, dc.relax_case("rowlen33"))
    n = _level_rows(mi, amg, 0)
    for rtype, nvec in ((18, 2), (16, 2), (40, 3), (8, 5), (8, 1)):
        with pytest.raises(mi.HypreError, match="RelaxLevelMulti"):
            amg.relax_level_multi(0, rtype, 0, np.zeros((nvec, n)), np.zeros((nvec, n)))
        mi.call("HYPRE_ClearAllErrors")


# ---------------------------------------------------------------- 3. cycle
def _laplace(n):
    import scipy.sparse as sp

    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n))
    I = sp.eye(n)
    A = (sp.kron(sp.kron(I, I), T) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(T, I), I)).tocsr()
    A.sort_indices()
    return A


HIERARCHIES = {
    "convdiff12": (lambda: convection_diffusion_3d(12), {}),
    "laplace16": (lambda: _laplace(16), {}),
    "laplace16-w": (lambda: _laplace(16), dict(cycle_type=2)),
    "laplace16-order0": (lambda: _laplace(16), dict(relax_order=0)),
    "laplace16-agg1": (lambda: _laplace(16), dict(agg_num_levels=1)),
    "laplace16-fp32": (lambda: _laplace(16), dict(mi_value_storage=1)),
    "convdiff12-air": (lambda: convection_diffusion_3d(12), dict(restriction=1)),
}


def _amg_iterations(mi, amg):
    it = mi.c_int()
    mi.call("HYPRE_BoomerAMGGetNumIterations", amg.h, mi.C.byref(it))
    return it.value


@pytest.mark.parametrize("name", list(HIERARCHIES))
def test_cycle(mi, width, name):
    make, kw = HIERARCHIES[name]
    M = make()
    N = M.shape[0]
    A = mi.matrix_from_scipy(M)
    rng = np.random.default_rng(len(name))
    for ncomp in (3, 5):
        B, X0 = rng.standard_normal((ncomp, N)), rng.standard_normal((ncomp, N))
        for max_iter, tol in ((1, 0.0), (3, 1e-12)):
            amg = mi.BoomerAMG(print_level=0, max_iterations=max_iter, tolerance=tol, **kw)
            amg.setup(A)
            got = {}
            for wd in (4, 1):
                width(wd)
                b, x = mi.IJVector(0, N - 1, B, ncomp=ncomp), mi.IJVector(0, N - 1, X0, ncomp=ncomp)
                c0 = {k: mi.counter(k) for k in ("mv_batched_cycles", "mv_fallback_cycles")}
                amg.solve(A, b, x)
                its = _amg_iterations(mi, amg)
                assert its == max_iter
                batched = mi.counter("mv_batched_cycles") - c0["mv_batched_cycles"]
                looped = mi.counter("mv_fallback_cycles") - c0["mv_fallback_cycles"]
                assert (batched, looped) == ((its * ((ncomp + 3) // 4), 0) if wd == 4 else (0, its)), (name, ncomp, wd)
                got[wd] = x.get_all()
            assert same(got[4], got[1]), (name, ncomp, max_iter, first_difference(got[4], got[1]))
            assert np.isfinite(got[4]).all() and not same(got[4], X0)


# ---------------------------------------------------------------- 4. Krylov
def _krylov(mi, method):
    if method == "gmres":
        return mi.GMRES(tolerance=1e-9, max_iterations=60, kspace=20, print_level=0)
    if method == "fgmres":
        return mi.FlexGMRES(tolerance=1e-9, max_iterations=60, kspace=20, print_level=0)
    if method == "cogmres":
        return mi.COGMRES(tolerance=1e-9, max_iterations=60, kspace=20, print_level=0, cgs=2)
    if method == "bicgstab":
        return mi.BiCGSTAB(tolerance=1e-9, max_iterations=60, print_level=0)
    return mi.PCG(tolerance=1e-9, max_iterations=60, print_level=0)


def _krylov_runs(mi, width, method, M, B, **amg_kw):
    """the solve with width 4 and with width 1: (iterations, history, x, counter deltas) each"""
    N = M.shape[0]
    A = mi.matrix_from_scipy(M)
    out = {}
    for wd in (4, 1):
        width(wd)
        b = mi.IJVector(0, N - 1, B, ncomp=len(B))
        x = mi.IJVector(0, N - 1, np.zeros_like(B), ncomp=len(B))
        amg = mi.BoomerAMG(print_level=0, **amg_kw)
        s = _krylov(mi, method)
        s.set_precond(amg)
        s.setup(A, b, x)
        names = ("mv_batched_cycles", "mv_batched_matvecs", "mv_fallback_cycles", "precond_cycles")
        c0 = {k: mi.counter(k) for k in names}
        assert s.solve(A, b, x) == 0
        out[wd] = (s.num_iterations, np.array(s.residual_history()), x.get_all(), {k: mi.counter(k) - c0[k] for k in names})
    return out


@pytest.mark.parametrize("method", ["gmres", "fgmres", "cogmres", "bicgstab", "pcg"])
def test_krylov(mi, width, method):
    if method == "pcg":
        M = _laplace(16)
        B = np.random.default_rng(16).standard_normal((3, M.shape[0]))
    else:
        M = convection_diffusion_3d(12)
        B, _ = three_component_rhs(M)
    r = _krylov_runs(mi, width, method, M, B)
    (it4, h4, x4, c4), (it1, h1, x1, c1) = r[4], r[1]
    assert it4 == it1 and 0 < it4 < 60
    assert same(h4, h1), first_difference(h4, h1)
    assert same(x4, x1), first_difference(x4, x1)
    assert c4["precond_cycles"] == c1["precond_cycles"] > 0 and c4["precond_cycles"] % 3 == 0
    assert c4["mv_batched_cycles"] == c4["precond_cycles"] // 3 and c4["mv_fallback_cycles"] == 0
    assert c4["mv_batched_matvecs"] > 0
    assert c1["mv_batched_cycles"] == 0 and c1["mv_batched_matvecs"] == 0 and c1["mv_fallback_cycles"] == c1["precond_cycles"] // 3


def _child(width_, **env):
    e = dict(os.environ)
    e.update({k: str(v) for k, v in env.items()})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mv_batch_worker.py"), str(width_)], env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_krylov_through_boomeramg_solve_and_with_poisoned_allocations():
    """Fresh processes (the switches are read once).  MI_HYPRE_GMRES_PERMUTED=0: the preconditioner is
    HYPRE_BoomerAMGSolve itself, which gathers and scatters the batch.  MI_HYPRE_POISON_ALLOC=1: every device block is
    handed out full of 0xFF bytes -- the Krylov vectors, the operators and every work array a batched pass touches.  (The
    levels' batch vectors themselves are zeroed when they are allocated, as Setup zeroes the levels' own vectors: for
    those this run shows no more than it shows for the single-vector cycle.)"""
    a, b = _child(4, MI_HYPRE_GMRES_PERMUTED=0), _child(1, MI_HYPRE_GMRES_PERMUTED=0)
    assert a["iters"] == b["iters"] and a["hist"] == b["hist"] and a["x"] == b["x"]
    assert a["counters"]["precond_cycles"] == b["counters"]["precond_cycles"] > 0
    assert a["counters"]["mv_batched_cycles"] > 0 and b["counters"]["mv_batched_cycles"] == 0
    ref, poisoned = _child(4), _child(4, MI_HYPRE_POISON_ALLOC=1)
    assert ref["counters"]["mv_batched_cycles"] > 0 and ref["counters"] == poisoned["counters"]
    assert ref["iters"] == poisoned["iters"] and ref["hist"] == poisoned["hist"] and ref["x"] == poisoned["x"]


# ---------------------------------------------------------------- 5. fallbacks
@pytest.mark.parametrize("kw", [dict(relax_type=18), dict(relax_type=11), dict(relax_type=16), dict(relax_type=40),
                                dict(smooth_type=5, smooth_num_levels=1)], ids=lambda kw: "-".join(map(str, kw.values())))
def test_fallbacks(mi, width, kw):
    """outside the hybrid Gauss-Seidel family the cycle takes the components one by one, whatever the width"""
    M = convection_diffusion_3d(12)
    B, _ = three_component_rhs(M)
    r = _krylov_runs(mi, width, "gmres", M, B, **kw)
    (it4, h4, x4, c4), (it1, h1, x1, c1) = r[4], r[1]
    assert it4 == it1 and same(h4, h1) and same(x4, x1), (first_difference(h4, h1), first_difference(x4, x1))
    assert c4["mv_batched_cycles"] == 0 and c1["mv_batched_cycles"] == 0
    assert c4["mv_fallback_cycles"] > 0 and c1["mv_fallback_cycles"] > 0
    assert c4["precond_cycles"] == c1["precond_cycles"]


# ---------------------------------------------------------------- 7. driver
def test_driver_key(tmp_path):
    """hypre_app on a 3-component deck with segregated_solve: 0 (built as tests/test_gpu_app.py builds its own):
    mi_multivector_batch 1 against 4 -- the same iteration count and identical solution files"""
    from tests.test_gpu_app import DEFAULT_AMG, _run, _write_mm_matrix, _write_mm_vector
    import scipy.sparse.linalg as spl

    A = convection_diffusion_3d(10)
    B, _ = three_component_rhs(A)
    lu = spl.splu(A.tocsc())
    out, files = {}, {}
    for wd in (1, 4):
        d = tmp_path / f"w{wd}"
        d.mkdir()
        _write_mm_matrix(d / "mat.mm", A)
        for c in range(3):
            _write_mm_vector(d / f"rhs{c}.mm", B[c])
            _write_mm_vector(d / f"sln{c}.mm", lu.solve(B[c]))
        vec = "".join(f"  rhs_file{c}: rhs{c}.mm\n  sln_file{c}: sln{c}.mm\n" for c in range(3))
        out[wd] = _run(d, f"""
linear_system:
  type: matrix_market
  matrix_file: mat.mm
{vec}  num_components: 3
  segregated_solve: 0
  rtol: 1.0e-6
  atol: 1.0e-8
  write_solution: true

solver_settings:
  method: bicg
  preconditioner: boomeramg
  tolerance: 1.0e-11
  max_iterations: 100
  print_level: 0
  mi_multivector_batch: {wd}
""" + DEFAULT_AMG)
        assert out[wd].count("allClose=1") == 3 and "allClose=0" not in out[wd], out[wd][-3000:]
        files[wd] = [(d / f"IJV{c}.sln.00000").read_bytes() for c in range(3)]
    solves = {wd: re.findall(r"Solve (\d+) : (\d+) iterations, final relative residual ([0-9.eE+-]+)", out[wd]) for wd in out}
    assert len(solves[1]) == 1 and solves[1] == solves[4], solves
    assert files[1] == files[4]
