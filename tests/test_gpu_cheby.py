"""GPU: Chebyshev relaxation (relax type 16) against the numpy restatement of tests/cheby_ref.py:
the eigenvalue bounds of every level, one sweep of every order on every level (and its zero-guess route, bit for bit),
every instantiation of the fused step, solves (GMRES, PCG, V / W, the coarse-tail switches, poisoned allocations), the
slot routes, refusals, a parameter change after Setup, the driver, and 2 / 3 ranks sharing the GPU."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from tests import cheby_ref
from tests import dict_cases as dc
from tests.test_cheby_spec import PLAIN, REF_GAP, XC, laplace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV_WORKER = os.path.join(ROOT, "tests", "cheby_env_worker.py")
DIST_WORKER = os.path.join(ROOT, "tests", "cheby_dist_worker.py")

pytestmark = pytest.mark.gpu

# the device's CG-Lanczos estimate against the restatement's: 100 x the float64-against-longdouble gap of the restatement
# itself (tests/test_cheby_spec.py, 2.84e-15), no less than 1e-13 -- the device sums its dots and rows in another order
CG_TOL = max(100.0 * REF_GAP, 1e-13)
SWEEP_TOL = 1e-12  # x max|ref|, as tests/test_gpu_fsai.py::test_smooth_level_step


def _level(amg, level):
    ia, ja, a, shape = amg.level_csr(level, 0)
    return sp.csr_matrix((a, ja, ia), shape=shape)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _problem(mi, case):
    n, stencil = (12, 7) if case == "lap7" else (10, 27)
    return mi.build_laplace_system(n, n, n, stencil)


def _check_sweeps(amg, level, B, theta, delta, rng, orders=(1, 2, 3, 4), diag=None):
    """RelaxLevel(level, 16) for the orders against the restatement, and the zero-guess route against the general one
    fed an explicit zero vector, bit for bit.  Returns the largest error over max|ref|."""
    n = B.shape[0]
    worst = 0.0
    for order in orders:
        amg.set_cheby(cheby_order=order)
        f, u = rng.standard_normal(n), rng.standard_normal(n)
        got = amg.relax_level(level, 16, 0, f, u)
        ref = cheby_ref.sweep(B, f, u, theta, delta, order, diag=diag)
        err = np.abs(got - ref).max() / np.abs(ref).max()
        worst = max(worst, err)
        assert err <= SWEEP_TOL, (level, order, err)
        zero = amg.relax_pair_level(level, 16, 1, f)  # u None: relax(.., u_is_zero)
        general = amg.relax_level(level, 16, 0, f, np.zeros(n))
        assert np.array_equal(_bits(zero), _bits(general)), (level, order)
        ref0 = cheby_ref.sweep(B, f, None, theta, delta, order, diag=diag)
        assert np.abs(zero - ref0).max() <= SWEEP_TOL * np.abs(ref0).max()
    return worst


@pytest.mark.parametrize("case", ["lap7", "lap27"])
@pytest.mark.parametrize("est", [0, 10])
def test_bounds_and_sweeps_on_every_level(mi, case, est):
    """level_cheby of every level against the restatement on level_csr: Gershgorin to 1e-14 relative (observed on one
    MI355X, 2026-10-19: 4.2e-16 on the 7-point, 2.0e-16 on the 27-point hierarchy), the CG bounds to CG_TOL = 2.84e-13
    relative to lambda_max (observed: 6.3e-16 and 4.3e-16); then one sweep of every order on every level."""
    A, b, x, rhs = _problem(mi, case)
    amg = mi.BoomerAMG(print_level=0, relax_type=16, cheby_eig_est=est)
    amg.setup(A)
    nlev = amg.num_levels
    assert nlev >= 3
    rng = np.random.default_rng(5)
    gap = 0.0
    for lev in range(nlev):
        B = _level(amg, lev)
        got = amg.level_cheby(lev)
        ref = cheby_ref.level_bounds(B, est)
        tol = 1e-14 if est == 0 else CG_TOL
        for key in ("eig_min", "eig_max", "lower", "upper", "theta", "delta"):
            g = abs(got[key] - ref[key]) / abs(ref["eig_max"])
            gap = max(gap, g)
            assert g <= tol, (lev, key, got[key], ref[key])
        _check_sweeps(amg, lev, B, got["theta"], got["delta"], rng)
    print(f"{case} eig_est {est}: largest relative gap of the bounds over {nlev} levels {gap:.2e}")


def _one_level(mi, M, **kw):
    A = mi.matrix_from_scipy(sp.csr_matrix(M))
    amg = mi.BoomerAMG(print_level=0, down_relax_type=16, up_relax_type=16, coarse_relax_type=16, max_levels=1, **kw)
    amg.setup(A)
    return A, amg


def _ran(mi, level):
    return mi.profile_kernel_name(mi.PROF_LVL_RELAX + level)


def _held(amg, level):
    return {0: "fp64", 2: "fp64", 8: "dict", 1: "fp32"}[amg.level_value_storage(level, 0)[0]]


def _expected(B, held):
    mean = B.nnz / B.shape[0]
    if mean < 3:
        return PLAIN[held]
    return XC[(4096 if mean >= 100 else 2048, held)]


def _long_row_operator(n=3000, length=2500, seed=2, pairs_only=False):
    """a 1-D Laplacian pattern (pairs_only: rows coupled in pairs, mean row length 2) plus one row and column of
    `length` entries, made SPD by diagonal dominance"""
    rng = np.random.default_rng(seed)
    if pairs_only:
        off = np.where(np.arange(n - 1) % 2 == 0, -1.0, 0.0)
        M = sp.diags([off, off], [-1, 1], shape=(n, n)).tocsr()
        M.eliminate_zeros()
        M = M.tolil()
    else:
        M = sp.diags([-1.0, -1.0], [-1, 1], shape=(n, n)).tolil()
    r = n // 2
    cols = rng.choice(n, size=length, replace=False)
    for c in cols:
        if c != r:
            M[r, c] = M[c, r] = -rng.random() - 0.1
    M = M.tocsr()
    return (M + sp.diags(abs(M).sum(axis=1).A1 * 1.05 + 0.1)).tocsr()


@pytest.mark.parametrize("case", ["plain", "xc", "dict", "wide", "long_row", "plain_long_row"])
def test_every_instantiation_ran(mi, case):
    """each operator runs the instantiation cheby_kernel_choice names for it, and the sweep equals the restatement;
    with a dictionary the result is that of the plain stream, bit for bit"""
    if case == "plain":
        M = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(4000, 4000)).tocsr()
    elif case == "xc":
        M = laplace(10, 27)
    elif case == "dict":
        M = laplace(22, 7)
    elif case == "wide":
        M = dc.relax_case("wide")
    elif case == "long_row":
        M = _long_row_operator()
    else:
        M = _long_row_operator(n=8000, pairs_only=True)
    rng = np.random.default_rng(8)
    n = M.shape[0]
    f, u = rng.standard_normal(n), rng.standard_normal(n)
    results = {}
    dict_modes = (True, False) if case in ("dict", "wide") else (True,)
    try:
        for with_dict in dict_modes:
            mi.set_value_dictionary(with_dict)
            A, amg = _one_level(mi, M)
            B = _level(amg, 0)
            held = _held(amg, 0)
            if case in ("dict", "wide"):
                assert B.nnz >= 65536 and dc.distinct(B) <= 256
                assert held == ("dict" if with_dict else "fp64")
            if case.startswith("plain"):
                assert B.nnz / n < 3
            if case == "wide":
                assert B.nnz / n >= 100
            if case.endswith("long_row"):
                assert np.diff(B.indptr).max() > 2048
            bd = amg.level_cheby(0)
            mi.profile_enable(mi.PROF_LVL_RELAX + 0)
            for order in (1, 3):
                amg.set_cheby(cheby_order=order)
                got = amg.relax_level(0, 16, 0, f, u)
                assert _ran(mi, 0) == _expected(B, held) == mi.cheby_kernel_choice(
                    xcache=B.nnz / n >= 3, tile_entries=4096 if B.nnz / n >= 100 else 2048, dictionary=held == "dict")
                ref = cheby_ref.sweep(B, f, u, bd["theta"], bd["delta"], order)
                assert np.abs(got - ref).max() <= SWEEP_TOL * np.abs(ref).max(), (case, order)
                results[(with_dict, order)] = got
    finally:
        mi.set_value_dictionary(True)
    if len(dict_modes) == 2:
        for order in (1, 3):
            assert np.array_equal(_bits(results[(True, order)]), _bits(results[(False, order)]))


def test_fp32_value_storage(mi):
    """levels >= 1 of the 27-point hierarchy with fp32 value storage: mode 1 (floats) and mode 2 (fp64 holding the
    rounded values) run their own instantiations and give the same bits; both equal the restatement on the rounded
    operator (the divisor stays the diagonal Setup computed before the values were narrowed)."""
    A, b, x, rhs = _problem(mi, "lap27")
    amgs = {m: mi.BoomerAMG(print_level=0, relax_type=16, mi_value_storage=m) for m in (0, 1, 2)}
    for a in amgs.values():
        a.setup(A)
    rng = np.random.default_rng(4)
    nlev = amgs[0].num_levels
    seen = 0
    for lev in range(1, nlev):
        B = _level(amgs[2], lev)
        diag = _level(amgs[0], lev).diagonal()
        n = B.shape[0]
        f, u = rng.standard_normal(n), rng.standard_normal(n)
        out = {}
        for m in (1, 2):
            if amgs[m].level_value_storage(lev, 0)[0] not in (1, 2, 8):
                continue
            bd = amgs[m].level_cheby(lev)
            mi.profile_enable(mi.PROF_LVL_RELAX + lev)
            out[m] = amgs[m].relax_level(lev, 16, 0, f, u)
            assert _ran(mi, lev) == _expected(B, _held(amgs[m], lev)), (lev, m)
            ref = cheby_ref.sweep(B, f, u, bd["theta"], bd["delta"], 2, diag=diag)
            assert np.abs(out[m] - ref).max() <= SWEEP_TOL * np.abs(ref).max(), (lev, m)
        if len(out) == 2:
            assert np.array_equal(_bits(out[1]), _bits(out[2])), lev
            seen += 1
    assert seen >= 1


def test_solves(mi):
    """GMRES(10) and PCG, orders 1 to 4, both estimates, V and W cycles: tests/cheby_env_worker.py asserts convergence
    within 100 iterations, the recomputed residual and PCG's residual history; the iteration counts are printed."""
    from tests import cheby_env_worker as w

    out = w.solve_matrix(mi)
    assert len(out) == 32
    print({k: v["iters"] for k, v in out.items()})


def _child(mode, **env):
    e = dict(os.environ, **{k: str(v) for k, v in env.items()})
    p = subprocess.run([sys.executable, ENV_WORKER, mode], env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


@pytest.fixture(scope="module")
def child_reference():
    ref = _child("few")
    assert len(ref) == 8
    return ref


@pytest.mark.parametrize("name,value,same", [("MI_HYPRE_TAIL_GRAPH", 0, True), ("MI_HYPRE_POISON_ALLOC", 1, True),
                                             ("MI_HYPRE_DENSE_TAIL_ROWS", 0, False), ("MI_HYPRE_LOCALITY_ORDER", 1, False)])
def test_solves_under_the_process_wide_switches(child_reference, name, value, same):
    """the same solves in a child process (the worker asserts convergence and the recomputed residual): without the
    captured graph of the collapsed coarse tail and with poisoned allocations the results are bit-identical to the
    default's (d is never read before step 0 wrote it); with the collapsed tail off and in the locality numbering they
    converge"""
    r = _child("few", **{name: value})
    assert r.keys() == child_reference.keys()
    if same:
        for key in child_reference:
            assert r[key] == child_reference[key], (name, key)


def test_slot_routes(mi):
    A, b, x, rhs = _problem(mi, "lap7")
    L = laplace(12)
    for slots in ((8, 8, 16), (16, 16, 9)):
        amg = mi.BoomerAMG(print_level=0, down_relax_type=slots[0], up_relax_type=slots[1], coarse_relax_type=slots[2])
        gm = mi.GMRES(tolerance=1e-8, max_iterations=100, kspace=10, print_level=0)
        gm.set_precond(amg)
        x.fill(0.0)
        gm.setup(A, b, x)
        assert gm.solve(A, b, x) == 0
        res = np.linalg.norm(rhs - L @ x.get()) / np.linalg.norm(rhs)
        assert res <= 1e-8 * (1 + 1e-6) and gm.num_iterations <= 100, (slots, res)
        assert amg.level_cheby(amg.num_levels - 1)["upper"] > 0.0  # every level has the data, the coarsest too


def test_refusals(mi):
    A, b, x, rhs = mi.build_laplace_system(8, 8, 8, 7)
    for kw in (dict(cheby_order=0), dict(cheby_order=5), dict(cheby_fraction=0.0), dict(cheby_fraction=1.0),
               dict(cheby_eig_est=-1), dict(cheby_variant=1), dict(cheby_scale=0)):
        amg = mi.BoomerAMG(print_level=0, relax_type=16, **kw)
        with pytest.raises(mi.HypreError, match="not implemented.*refusing to"):
            amg.setup(A)
        mi.call("HYPRE_ClearAllErrors")
    M = laplace(6).tolil()
    M[7, 7] = -6.0
    Abad = mi.matrix_from_scipy(M.tocsr())
    amg = mi.BoomerAMG(print_level=0, down_relax_type=16, up_relax_type=16, coarse_relax_type=16, max_levels=1)
    with pytest.raises(mi.HypreError, match="diagonal entry that is not positive.*not.*implemented.*refusing to"):
        amg.setup(Abad)
    mi.call("HYPRE_ClearAllErrors")
    plain = mi.BoomerAMG(print_level=0)
    plain.setup(A)
    n = 512
    with pytest.raises(mi.HypreError, match="returned 4"):
        plain.relax_level(0, 16, 0, np.ones(n), np.zeros(n))
    mi.call("HYPRE_ClearAllErrors")
    with pytest.raises(mi.HypreError):
        plain.level_cheby(0)
    mi.call("HYPRE_ClearAllErrors")
    good = mi.BoomerAMG(print_level=0, relax_type=16)
    good.setup(A)
    assert good.level_cheby(0)["upper"] > 0.0


def test_parameter_change_after_setup(mi):
    """SetChebyOrder between two solves changes the sweep (and the collapsed tail): the second solve equals that of a
    fresh Setup with the new order, and one RelaxLevel equals the restatement with it"""
    A, b, x, rhs = _problem(mi, "lap7")

    def solve(amg, gm=None):
        x.fill(0.0)
        if gm is None:
            gm = mi.GMRES(tolerance=1e-8, max_iterations=100, kspace=10, print_level=0)
            gm.set_precond(amg)
            gm.setup(A, b, x)
        gm.solve(A, b, x)
        return gm, gm.num_iterations, x.get()

    amg = mi.BoomerAMG(print_level=0, relax_type=16, cheby_order=1)
    gm, i1, x1 = solve(amg)
    fresh = mi.BoomerAMG(print_level=0, relax_type=16, cheby_order=3)
    _, i3, x3 = solve(fresh)
    before = amg.level_cheby(0)
    amg.set_cheby(cheby_order=3)
    _, i13, x13 = solve(amg, gm)  # no new Setup
    assert i13 == i3 and np.array_equal(_bits(x13), _bits(x3))
    assert i3 < i1
    assert amg.level_cheby(0) == before  # the bounds do not depend on the order: not estimated again
    B = _level(amg, 0)
    rng = np.random.default_rng(1)
    f, u = rng.standard_normal(B.shape[0]), rng.standard_normal(B.shape[0])
    got = amg.relax_level(0, 16, 0, f, u)
    ref = cheby_ref.sweep(B, f, u, before["theta"], before["delta"], 3)
    assert np.abs(got - ref).max() <= SWEEP_TOL * np.abs(ref).max()
    # another estimate: the bounds are rebuilt at the next use
    amg.set_cheby(cheby_eig_est=0)
    want = cheby_ref.level_bounds(B, 0)
    assert abs(amg.level_cheby(0)["upper"] - want["upper"]) <= 1e-14 * want["upper"]


@pytest.mark.parametrize("keys", ["", "  mi_cheby_order: 3\n  mi_cheby_fraction: 0.25\n  mi_cheby_eig_est: 0\n"])
def test_driver_runs_the_cheby_input(tmp_path, keys):
    from tests.test_gpu_app import _run

    text = open(os.path.join(ROOT, "hypre-mini-app_amd", "etc", "laplace_3d_cheby.yaml")).read()
    assert "relax_type: 16" in text
    text = re.sub(r"(n[xyz]): 64", r"\1: 16", text) + keys
    out = _run(tmp_path, text)
    m = re.search(r"max \|x - 1\| = ([0-9.eE+-]+)", out)
    assert m and float(m.group(1)) < 1e-6, out[-2000:]


@pytest.mark.parametrize("nproc,n,seq,empty", [(2, 12, -1, 0), (3, 10, 0, 0), (3, 8, -1, 1)])
def test_cheby_on_ranks_sharing_the_gpu(nproc, n, seq, empty):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MI_HYPRE_HOST_THREADS="2", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr",
           "127.0.0.1", "--master-port", str(30411 + nproc + n + 50 * empty), DIST_WORKER, "--grid", str(n), "--seq", str(seq),
           "--empty", str(empty)]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    assert p.stdout.count("cheby rank ok") == nproc, p.stdout[-4000:]
