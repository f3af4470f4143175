"""GPU: the FSAI smoother (smooth_type 4) and the standalone HYPRE_FSAI solver against the numpy restatement of
tests/fsai_ref.py ("FSAI"): G of every smoothed level, omega, one smoothing step, determinism,
PCG with FSAI, BoomerAMG with FSAI levels, parameter changes after Setup, refusals, the driver, and 2 / 3 ranks."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from tests import fsai_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "fsai_dist_worker.py")

pytestmark = pytest.mark.gpu


def _ij(mi, M):
    M = sp.csr_matrix(M)
    n = M.shape[0]
    A = mi.IJMatrix(0, n - 1)
    coo = M.tocoo()
    A.set_values_coo(coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data.astype(np.float64))
    A.assemble()
    return A


def _level_B(amg, level):
    ia, ja, a, shape = amg.level_csr(level, 0)
    return sp.csr_matrix((a, ja, ia), shape=shape)


def _level_G(amg, level):
    got = amg.level_fsai(level)
    assert got is not None, f"level {level} has no FSAI smoother"
    ia, ja, a, om = got
    n = len(ia) - 1
    return sp.csr_matrix((a, ja, ia), shape=(n, n)), om


def _ragged(n=2000, seed=12):
    """random nonsymmetric M-matrix, rows of 1 ... ~30 lower entries and one long row (~50 lower entries)."""
    rng = np.random.default_rng(seed)
    M = sp.random(n, n, density=0.012, random_state=rng, format="lil")
    for c in rng.choice(n - 1, size=40, replace=False):
        M[n - 1, c] = rng.standard_normal()
    M = M.tocsr()
    M.setdiag(0.0)
    M.eliminate_zeros()
    M = -abs(M)
    return (M + sp.diags(np.abs(M).sum(axis=1).A1 * 1.01 + 1e-3)).tocsr()


def _same_G(G, Gr):
    assert np.array_equal(G.indptr, Gr.indptr) and np.array_equal(G.indices, Gr.indices)
    err = np.abs(G.data - Gr.data).max()
    assert err <= 1e-12 * np.abs(Gr.data).max(), err


@pytest.mark.parametrize("case,k,theta,levels", [("lap7", 1, 0.01, 50), ("lap7", 2, 0.0, 1), ("lap7", 3, 0.3, 1),
                                                 ("lap27", 1, 0.0, 2), ("lap27", 1, 0.3, 3), ("ragged", 1, 0.0, 1),
                                                 ("ragged", 1, 0.3, 1)])
def test_g_and_omega_on_every_smoothed_level(mi, case, k, theta, levels):
    if case == "ragged":
        M = _ragged()
        A = _ij(mi, M)
    else:
        n = 12 if case == "lap7" else 10
        A, b, x, rhs = mi.build_laplace_system(n, n, n, 7 if case == "lap7" else 27)
    amg = mi.BoomerAMG(print_level=0, smooth_type=4, smooth_num_levels=levels, fsai_num_levels=k, fsai_threshold=theta)
    amg.setup(A)
    nlev = amg.num_levels
    assert nlev > 1
    seen = 0
    for lev in range(nlev):
        got = amg.level_fsai(lev)
        if lev >= min(levels, nlev - 1):
            assert got is None
            continue
        B = _level_B(amg, lev)
        G, om = _level_G(amg, lev)
        _same_G(G, fsai_ref.factor(B, theta, k))
        om_ref = fsai_ref.omega(G, B, 5)
        assert abs(om - om_ref) <= 1e-12 * om_ref, (om, om_ref)
        seen += 1
    assert seen == min(levels, nlev - 1)
    if case == "ragged" and theta == 0.0:  # every group size of the local-solve kernel ran
        m = np.diff(_level_G(amg, 0)[0].indptr)
        assert m.max() > 32 and ((m > 16) & (m <= 32)).any() and (m <= 16).any()


def test_g_in_the_locality_numbering_of_level_0(mi, monkeypatch):
    """With the internal locality numbering on, G of level 0 belongs to the level's stored ordering (GetLevelCSR's)."""
    monkeypatch.setenv("MI_HYPRE_LOCALITY_ORDER", "1")
    A, b, x, rhs = mi.build_laplace_system(12, 12, 12, 7)
    amg = mi.BoomerAMG(print_level=0, smooth_type=4, smooth_num_levels=2)
    amg.setup(A)
    applied, order = amg.input_ordering()
    assert applied and not np.array_equal(order, np.arange(len(order)))
    for lev in (0, 1):
        B = _level_B(amg, lev)
        G, om = _level_G(amg, lev)
        _same_G(G, fsai_ref.factor(B, 0.01, 1))
        om_ref = fsai_ref.omega(G, B, 5)
        assert abs(om - om_ref) <= 1e-12 * om_ref


def test_smooth_level_step(mi):
    A, b, x, rhs = mi.build_laplace_system(10, 10, 10, 7)
    amg = mi.BoomerAMG(print_level=0, smooth_type=4, smooth_num_levels=2)
    amg.setup(A)
    rng = np.random.default_rng(3)
    for lev in (0, 1):
        B = _level_B(amg, lev)
        G, om = _level_G(amg, lev)
        f = rng.standard_normal(B.shape[0])
        u0 = rng.standard_normal(B.shape[0])
        for u in (None, u0):
            got = amg.smooth_level(lev, f, u)
            ref = fsai_ref.smooth(G, om, B, f, u)
            assert np.allclose(got, ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())


def test_g_is_bit_identical_across_setups(mi):
    A = _ij(mi, _ragged(seed=5))
    gs = []
    for _ in range(2):
        amg = mi.BoomerAMG(print_level=0, smooth_type=4, smooth_num_levels=1)
        amg.setup(A)
        gs.append(amg.level_fsai(0))
    for u, v in zip(gs[0], gs[1]):
        assert np.array_equal(np.asarray(u), np.asarray(v))


def test_standalone_pcg_with_fsai_matches_numpy(mi):
    n = 24
    A, b, x, rhs = mi.build_laplace_system(n, n, n, 7)
    fs = mi.FSAI()
    pcg = mi.PCG(tolerance=1e-8, max_iterations=200, print_level=0)
    pcg.set_precond(fs)
    pcg.setup(A, b, x)
    assert pcg.solve(A, b, x) == 0
    # numpy PCG (krylov/pcg.c, two_norm 0) with the restated G and omega
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n))
    I = sp.identity(n)
    L = (sp.kron(sp.kron(I, I), T) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(T, I), I)).tocsr()
    G = fsai_ref.factor(L, 0.01, 1)
    om = fsai_ref.omega(G, L, 5)
    prec = lambda r: om * (G.T @ (G @ r))  # noqa: E731
    bb = rhs.copy()
    xx = np.zeros_like(bb)
    bi = prec(bb) @ bb
    r = bb - L @ xx
    p = prec(r)
    gamma = r @ p
    norms = [np.sqrt(abs(gamma) / bi)]
    it = 0
    while it < 200:
        it += 1
        s = L @ p
        alpha = gamma / (s @ p)
        xx += alpha * p
        r -= alpha * s
        z = prec(r)
        gold, gamma = gamma, r @ z
        norms.append(np.sqrt(abs(gamma) / bi))
        if gamma / bi < 1e-16:
            break
        p = z + (gamma / gold) * p
    assert pcg.num_iterations == it
    assert np.allclose(pcg.residual_history(), norms, rtol=1e-8, atol=1e-14)
    assert np.abs(x.get() - 1.0).max() < 1e-6


@pytest.mark.parametrize("levels,cycle,sweeps", [(1, 1, 1), (3, 1, 1), (50, 1, 1), (3, 2, 1), (50, 1, 2)])
def test_gmres_with_fsai_levels_converges(mi, levels, cycle, sweeps):
    A, b, x, rhs = mi.build_laplace_system(20, 20, 20, 7)
    amg = mi.BoomerAMG(print_level=0, smooth_type=4, smooth_num_levels=levels, cycle_type=cycle, num_sweeps=sweeps)
    gm = mi.GMRES(tolerance=1e-8, max_iterations=100, kspace=50, print_level=0)
    gm.set_precond(amg)
    gm.setup(A, b, x)
    assert gm.solve(A, b, x) == 0
    assert gm.final_rel_res < 1e-8 and np.abs(x.get() - 1.0).max() < 1e-6


def _gmres_solution(mi, A, b, x, amg, keep=None):
    x.fill(0.0)
    gm = mi.GMRES(tolerance=1e-8, max_iterations=100, kspace=50, print_level=0)
    gm.set_precond(amg)
    gm.setup(A, b, x)
    gm.solve(A, b, x)
    if keep is not None:
        keep.append(gm)
    return gm.num_iterations, x.get()


def test_smooth_type_4_without_levels_changes_nothing(mi):
    A, b, x, rhs = mi.build_laplace_system(14, 14, 14, 7)
    i0, x0 = _gmres_solution(mi, A, b, x, mi.BoomerAMG(print_level=0))
    i1, x1 = _gmres_solution(mi, A, b, x, mi.BoomerAMG(print_level=0, smooth_type=4, smooth_num_levels=0))
    assert i0 == i1 and np.array_equal(x0, x1)


def test_fsai_parameter_change_after_setup(mi):
    """Changing an FSAI parameter after Setup changes the next solve as a fresh Setup with it does (smoothers and the
    collapsed coarse tail are rebuilt)."""
    A, b, x, rhs = mi.build_laplace_system(14, 14, 14, 7)
    amg = mi.BoomerAMG(print_level=0, smooth_type=4, smooth_num_levels=50)
    keep = []
    i0, x0 = _gmres_solution(mi, A, b, x, amg, keep)
    G0 = amg.level_fsai(0)
    amg2 = mi.BoomerAMG(print_level=0, smooth_type=4, smooth_num_levels=50)
    amg2.set_fsai(fsai_threshold=0.3, fsai_eig_max_iters=3)
    i2, x2 = _gmres_solution(mi, A, b, x, amg2)
    amg.set_fsai(fsai_threshold=0.3, fsai_eig_max_iters=3)
    x.fill(0.0)
    gm = keep[0]
    gm.solve(A, b, x)  # no new Setup
    assert gm.num_iterations == i2 and np.allclose(x.get(), x2, rtol=0, atol=1e-13)
    G1, G2 = amg.level_fsai(0), amg2.level_fsai(0)
    assert G1[3] != G0[3]
    assert np.array_equal(G1[1], G2[1]) and np.array_equal(G1[2], G2[2]) and G1[3] == G2[3]


def test_refusals(mi):
    A, b, x, rhs = mi.build_laplace_system(8, 8, 8, 27)
    for kw, msg in ((dict(fsai_algo_type=1), "not implemented"), (dict(fsai_algo_type=2), "not implemented"),
                    (dict(fsai_num_levels=3), "limit is 64")):
        amg = mi.BoomerAMG(print_level=0, smooth_type=4, smooth_num_levels=1, **kw)
        with pytest.raises(mi.HypreError, match=msg):
            amg.setup(A)
        mi.call("HYPRE_ClearAllErrors")
    fs = mi.FSAI(algo_type=1)
    with pytest.raises(mi.HypreError, match="not implemented"):
        fs.setup(A)
    mi.call("HYPRE_ClearAllErrors")
    # y_last <= 0: an indefinite 2 x 2 block in rows 5, 6
    M = sp.diags(np.full(10, 4.0)).tolil()
    M[5, 5], M[6, 6], M[5, 6], M[6, 5] = 1.0, 1.0, 2.0, 2.0
    fs = mi.FSAI(threshold=0.0)
    with pytest.raises(mi.HypreError, match="row 6"):
        fs.setup(_ij(mi, M.tocsr()))
    mi.call("HYPRE_ClearAllErrors")


def test_driver_runs_smooth_type_4(tmp_path):
    from tests.test_gpu_app import _run

    out = _run(tmp_path, """
linear_system:
  type: laplace_3d
  nx: 20
  ny: 20
  nz: 20
  stencil: 7

solver_settings:
  method: gmres
  preconditioner: boomeramg
  tolerance: 1.0e-9
  max_iterations: 100
  kspace: 50
  print_level: 2

boomeramg_settings:
  print_level: 1
  coarsen_type: 8
  smooth_type: 4
  smooth_num_levels: 3
""")
    assert out.count("mi_hypre FSAI:") == 3, out[-2000:]
    m = re.search(r"max \|x - 1\| = ([0-9.eE+-]+)", out)
    assert m and float(m.group(1)) < 1e-6, out[-2000:]


@pytest.mark.parametrize("nproc,n,seq,empty", [(2, 12, -1, 0), (3, 10, 0, 0), (3, 8, -1, 1)])
def test_fsai_on_ranks_sharing_the_gpu(nproc, n, seq, empty):
    """empty = 1: the last rank owns no rows; standalone FSAI Setup and Solve on that partition against numpy."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MI_HYPRE_HOST_THREADS="2", OMP_NUM_THREADS="1",
               MI_HYPRE_LOCALITY_ORDER="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr",
           "127.0.0.1", "--master-port", str(30311 + nproc + n + 50 * empty), WORKER, "--grid", str(n), "--seq", str(seq), "--empty", str(empty)]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    assert p.stdout.count("fsai rank ok") == nproc, p.stdout[-4000:]
