"""GPU: the iterative ILU(0) setup (HYPRE_ILUSetIterativeSetupType 1-4 and BoomerAMG's iterative_ilu_* keys, DESIGN.md
section 3) against the numpy restatement of tests/itilu_ref.py: types 3 / 4 bit for bit, convergence of every type to
the exact factors, the stop option and the histories, GMRES with the ILU preconditioner and with ILU smoothers,
refusals, the driver, and 2 / 3 ranks."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from tests import itilu_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "itilu_dist_worker.py")

pytestmark = pytest.mark.gpu


def _ij(mi, M):
    M = sp.csr_matrix(M)
    n = M.shape[0]
    A = mi.IJMatrix(0, n - 1)
    coo = M.tocoo()
    A.set_values_coo(coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data.astype(np.float64))
    A.assemble()
    return A


_CASES = {}


def _case(name):
    if name not in _CASES:
        M = {"7pt": lambda: itilu_ref.laplace(10, 7), "27pt": lambda: itilu_ref.laplace(8, 27),
             "nonsym": lambda: itilu_ref.nonsymmetric(800)}[name]()
        _CASES[name] = (M, itilu_ref.Plan(M))
    return _CASES[name]


def _factors(mi, A, **kw):
    ilu = mi.ILU(**kw)
    ilu.setup(A)
    ia, ja, a = ilu.factors()
    return ilu, ia, ja, a


@pytest.mark.parametrize("name", ["7pt", "27pt", "nonsym"])
def test_synchronous_types_are_bit_identical_to_the_restatement(mi, name):
    M, P = _case(name)
    A = _ij(mi, M)
    for sweeps in (1, 2, 5):
        ref = P.run(sweeps)
        got = {}
        for typ, opt in ((3, 0), (4, 4 | 8 | 16), (3, 4 | 16)):
            ilu, ia, ja, a = _factors(mi, A, iterative_algorithm_type=typ, iterative_setup_option=opt,
                                      iterative_max_iterations=sweeps, trisolve=0)
            assert np.array_equal(ia, P.A.indptr) and np.array_equal(ja, P.A.indices)
            assert np.array_equal(a, ref), (typ, sweeps, np.abs(a - ref).max())
            assert ilu.iterative_setup_info()[0] == sweeps
            got[(typ, opt)] = a
            if opt & 16:  # the correction history of the restatement, bit for bit
                x, cs = P.start(), []
                for _ in range(sweeps):
                    xn = P.sweep(x)
                    cs.append(P.correction(x, xn))
                    x = xn
                corr, res = ilu.iterative_setup_history()
                assert np.array_equal(corr, np.array(cs))
                if opt & 8:
                    assert len(res) == sweeps and res[-1] == pytest.approx(P.residual(ref), rel=1e-12, abs=1e-300)
            ilu.destroy()
        # a second setup of the same kind gives the same bits
        _, _, _, again = _factors(mi, A, iterative_algorithm_type=3, iterative_max_iterations=sweeps)
        assert np.array_equal(again, got[(3, 0)])


@pytest.mark.parametrize("name", ["7pt", "27pt", "nonsym"])
def test_every_type_converges_to_the_exact_factors(mi, name):
    M, P = _case(name)
    A = _ij(mi, M)
    n = M.shape[0]
    _, _, _, exact = _factors(mi, A)
    assert np.abs(exact - itilu_ref.exact_ilu0(M)).max() <= 1e-14 * np.abs(exact).max()
    rng = np.random.default_rng(3)
    f = rng.standard_normal(n)

    def apply(**kw):
        ilu = mi.ILU(max_iterations=1, tolerance=0.0, **kw)
        b = mi.IJVector(0, n - 1, f.copy())
        x = mi.IJVector(0, n - 1, np.zeros(n))
        ilu.setup(A)
        ilu.solve(A, b, x)
        return ilu.factors()[2], x.get()

    _, y0 = apply()
    for typ in (1, 2, 3, 4):
        a, y = apply(iterative_algorithm_type=typ, iterative_max_iterations=80)
        assert np.abs(a - exact).max() <= 1e-12 * np.abs(exact).max(), (typ, np.abs(a - exact).max())
        assert np.abs(y - y0).max() <= 1e-10 * np.abs(y0).max(), typ


def test_stop_option_and_histories(mi):
    M, P = _case("27pt")
    A = _ij(mi, M)
    want = P.stop_sweep(1e-6, 100)
    assert 1 < want < 100
    ilu, _, _, a = _factors(mi, A, iterative_algorithm_type=3, iterative_setup_option=2 | 16,
                            iterative_max_iterations=100, iterative_tolerance=1e-6)
    sweeps, c, r = ilu.iterative_setup_info()
    assert sweeps == want and c <= 1e-6 and r == -1.0
    corr, res = ilu.iterative_setup_history()
    assert len(corr) == want and len(res) == 0 and corr[-2] > 1e-6
    assert np.array_equal(a, P.run(want))
    # the same with type 4 and type 2 (whose own correction decides): both stop once c <= tol
    for typ in (4, 2):
        ilu, _, _, _ = _factors(mi, A, iterative_algorithm_type=typ, iterative_setup_option=2,
                                iterative_max_iterations=100, iterative_tolerance=1e-6)
        sweeps, c, _ = ilu.iterative_setup_info()
        assert c <= 1e-6 and sweeps < 100 and (typ != 4 or sweeps == want)
    # without bit 2 exactly max_iter sweeps; the histories hold what the bits computed
    for opt, nc, nr in ((4 | 16, 7, 0), (8 | 16, 0, 7), (4 | 8 | 16, 7, 7), (4 | 8, 0, 0), (0, 0, 0), (32, 0, 0)):
        ilu, _, _, _ = _factors(mi, A, iterative_algorithm_type=3, iterative_setup_option=opt,
                                iterative_max_iterations=7, iterative_tolerance=1e-6)
        sweeps, c, r = ilu.iterative_setup_info()
        corr, res = ilu.iterative_setup_history()
        assert sweeps == 7 and len(corr) == nc and len(res) == nr, (opt, sweeps, len(corr), len(res))
        assert (c >= 0) == bool(opt & 4) and (r >= 0) == bool(opt & 8)


def _gmres(mi, A, n, precond, f):
    b = mi.IJVector(0, n - 1, f.copy())
    x = mi.IJVector(0, n - 1, np.zeros(n))
    gm = mi.GMRES(tolerance=1e-9, max_iterations=200, kspace=50, print_level=0)
    gm.set_precond(precond)
    gm.setup(A, b, x)
    gm.solve(A, b, x)
    return gm, x.get()


def test_gmres_with_the_iterative_ilu_preconditioner(mi):
    M = itilu_ref.laplace(12, 7)
    n = M.shape[0]
    A = _ij(mi, M)
    f = M @ np.ones(n)
    for tri in (0, 1):
        gm0, x0 = _gmres(mi, A, n, mi.ILU(trisolve=tri), f)
        h0 = gm0.residual_history()
        for sweeps in (3, 60):
            gm, x = _gmres(mi, A, n, mi.ILU(trisolve=tri, iterative_algorithm_type=3, iterative_max_iterations=sweeps), f)
            assert gm.final_rel_res < 1e-9 and np.abs(x - 1.0).max() < 1e-6, (tri, sweeps)
            if sweeps == 60:
                h = gm.residual_history()
                assert len(h) == len(h0) and np.abs(h - h0).max() <= 1e-8 * h0[0], (tri, np.abs(h - h0).max())


def test_boomeramg_with_iterative_ilu_smoothers(mi):
    A, b, x, rhs = mi.build_laplace_system(16, 16, 16, 7)
    kw = dict(print_level=0, smooth_type=5, smooth_num_levels=2, ilu_tri_solve=0)
    hist = {}
    for it in ({}, dict(iterative_ilu_algorithm_type=3, iterative_ilu_max_iterations=60),
               dict(iterative_ilu_algorithm_type=1, iterative_ilu_setup_option=2, iterative_ilu_max_iterations=100,
                    iterative_ilu_tolerance=1e-14), dict(iterative_ilu_algorithm_type=4, iterative_ilu_max_iterations=2)):
        amg = mi.BoomerAMG(**kw, **it)
        gm = mi.GMRES(tolerance=1e-9, max_iterations=100, kspace=50, print_level=0)
        gm.set_precond(amg)
        x.set(np.zeros(x.get().shape))
        gm.setup(A, b, x)
        gm.solve(A, b, x)
        assert gm.final_rel_res < 1e-9 and np.abs(x.get() - 1.0).max() < 1e-6, it
        hist[it.get("iterative_ilu_algorithm_type", 0), it.get("iterative_ilu_max_iterations", 0)] = gm.residual_history()
        gm.destroy()
        amg.destroy()
    h0 = hist[0, 0]
    for key in ((3, 60), (1, 100)):
        h = hist[key]
        assert len(h) == len(h0) and np.abs(h - h0).max() <= 1e-8 * h0[0], (key, np.abs(h - h0).max())


def test_a_changed_iterative_key_after_setup_rebuilds_the_smoothers(mi):
    A, b, x, rhs = mi.build_laplace_system(12, 12, 12, 7)
    amg = mi.BoomerAMG(print_level=0, smooth_type=5, smooth_num_levels=1, ilu_tri_solve=0, max_iterations=3,
                       tolerance=0.0, iterative_ilu_algorithm_type=3, iterative_ilu_max_iterations=1)
    amg.setup(A)

    def cycles():
        x.set(np.zeros(x.get().shape))
        mi.call("HYPRE_BoomerAMGSolve", amg.h, A.par, b.par, x.par, allow=(mi.HYPRE_ERROR_CONV,))
        return x.get()

    one = cycles()
    mi.call("HYPRE_BoomerAMGSetILUIterSetupMaxIter", amg.h, 40)
    forty = cycles()
    ref = mi.BoomerAMG(print_level=0, smooth_type=5, smooth_num_levels=1, ilu_tri_solve=0, max_iterations=3,
                       tolerance=0.0, iterative_ilu_algorithm_type=3, iterative_ilu_max_iterations=40)
    ref.setup(A)
    x.set(np.zeros(x.get().shape))
    mi.call("HYPRE_BoomerAMGSolve", ref.h, A.par, b.par, x.par, allow=(mi.HYPRE_ERROR_CONV,))
    assert not np.array_equal(one, forty) and np.array_equal(forty, x.get())


def test_refusals(mi):
    A = _ij(mi, itilu_ref.laplace(6, 7))
    for kw in (dict(iterative_algorithm_type=5), dict(iterative_algorithm_type=3, fill=1),
               dict(iterative_algorithm_type=3, ilu_type=1), dict(iterative_algorithm_type=3, iterative_setup_option=64)):
        ilu = mi.ILU(**kw)
        with pytest.raises(mi.HypreError, match="not implemented"):
            ilu.setup(A)
        mi.call("HYPRE_ClearAllErrors")
    B, b, x, rhs = mi.build_laplace_system(8, 8, 8, 7)
    for kw in (dict(iterative_ilu_algorithm_type=5), dict(iterative_ilu_algorithm_type=3, ilu_level=1),
               dict(iterative_ilu_algorithm_type=3, ilu_type=1)):
        amg = mi.BoomerAMG(print_level=0, smooth_type=5, smooth_num_levels=1, **kw)
        with pytest.raises(mi.HypreError, match="not implemented"):
            amg.setup(B)
        mi.call("HYPRE_ClearAllErrors")
    # a zero pivot names its row: row 2 stores no diagonal; row 4 stores a_44 = 0, which no sweep changes
    for typ in (3, 1):
        rows = [0, 1, 2, 3, 3, 4, 4, 5, 5]
        cols = [0, 1, 3, 2, 3, 4, 5, 4, 5]
        vals = [4.0, 4.0, 1.0, 1.0, 4.0, 4.0, 1.0, 1.0, 4.0]
        ilu = mi.ILU(iterative_algorithm_type=typ, iterative_max_iterations=3)
        with pytest.raises(mi.HypreError, match="row 2 "):
            ilu.setup(_ij(mi, sp.csr_matrix((vals, (rows, cols)), shape=(6, 6))))
        mi.call("HYPRE_ClearAllErrors")
        rows[2:], cols[2:] = [2, 2, 3, 3, 4, 4, 5, 5], [2, 3, 2, 3, 4, 5, 4, 5]
        vals[2:] = [4.0, 1.0, 1.0, 4.0, 0.0, 1.0, 1.0, 4.0]
        ilu = mi.ILU(iterative_algorithm_type=typ, iterative_max_iterations=3)
        with pytest.raises(mi.HypreError, match="row 4 "):
            ilu.setup(_ij(mi, sp.csr_matrix((vals, (rows, cols)), shape=(6, 6))))
        mi.call("HYPRE_ClearAllErrors")


_DECK = """
linear_system:
  type: laplace_3d
  nx: 16
  ny: 16
  nz: 16
  stencil: 7

solver_settings:
  method: gmres
  preconditioner: {precond}
  tolerance: 1.0e-9
  max_iterations: 300
  kspace: 50
  print_level: 0

"""


def test_driver_runs_iterative_ilu_decks(tmp_path):
    from tests.test_gpu_app import _run

    out = _run(tmp_path, _DECK.format(precond="ilu") + """ilu_preconditioner_settings:
  iterative_algorithm_type: 3
  iterative_ilu_max_iterations: 20
  trisolve: 0
""")
    assert "mi_hypre ILU iterative setup (type 3, option 2)" in out, out[-2000:]
    m = re.search(r"max \|x - 1\| = ([0-9.eE+-]+)", out)
    assert m and float(m.group(1)) < 1e-6, out[-2000:]
    out = _run(tmp_path, _DECK.format(precond="boomeramg") + """boomeramg_settings:
  print_level: 1
  coarsen_type: 8
  smooth_type: 5
  smooth_num_levels: 2
  ilu_tri_solve: 0
  iterative_ilu_algorithm_type: 4
  iterative_ilu_setup_option: 3
  iterative_ilu_max_iterations: 30
  iterative_ilu_tolerance: 1.0e-6
""")
    assert out.count("mi_hypre ILU iterative setup (type 4, option 3)") == 2, out[-2000:]
    m = re.search(r"max \|x - 1\| = ([0-9.eE+-]+)", out)
    assert m and float(m.group(1)) < 1e-6, out[-2000:]


@pytest.mark.parametrize("nproc,empty", [(2, 0), (3, 1)])
def test_iterative_ilu_on_ranks_sharing_the_gpu(nproc, empty):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MI_HYPRE_HOST_THREADS="2", OMP_NUM_THREADS="1",
               MI_HYPRE_LOCALITY_ORDER="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr",
           "127.0.0.1", "--master-port", str(30411 + nproc + 50 * empty), WORKER, "--grid", "8", "--empty", str(empty)]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    assert p.stdout.count("itilu rank ok") == nproc, p.stdout[-4000:]
