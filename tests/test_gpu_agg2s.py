"""GPU: aggressive levels with the two-stage extended interpolation (agg_interp_type 5) built on
the device -- second-generation graph, second PMIS, marker correction, stage operators, their product and the
truncations -- bit for bit the host-only setup of the same matrix; GMRES + AMG against multipass; the driver; two
ranks sharing the GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from tests.agg2s_common import host_amg, ij_host, random_mmatrix, zero_denominator_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "agg2s_dist_worker.py")

pytestmark = pytest.mark.gpu


def _pair(mi, name):
    """the same operator assembled for the device setup and for the host-only setup"""
    if name == "randmm":
        M = random_mmatrix()
        n = M.shape[0]
        A = mi.IJMatrix(0, n - 1)
        coo = M.tocoo()
        A.set_values_coo(coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data.astype(np.float64))
        A.assemble()
        return A, ij_host(mi, M)
    n, stencil = {"lap7_24": (24, 7), "lap27_16": (16, 27)}[name]
    return mi.build_laplace_system(n, n, n, stencil)[0], mi.build_laplace_system_host(n, n, n, stencil, 0, 1)[0]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _assert_bit_identical(dev, host, nagg):
    assert dev.num_levels == host.num_levels and dev.num_levels > 1
    assert nagg >= 1
    for l in range(dev.num_levels):
        for which in (0, 2, 3) if l < dev.num_levels - 1 else (0,):
            ia, ja, a, shape = dev.level_csr(l, which)
            hia, hja, ha, hshape = host.level_csr(l, which)
            assert shape == hshape, (l, which)
            assert np.array_equal(ia, hia) and np.array_equal(ja, hja), (l, which)
            assert np.array_equal(_bits(a), _bits(ha)), (l, which)
        if l < dev.num_levels - 1:
            assert np.array_equal(dev.level_cf(l), host.level_cf(l)), l
            assert np.array_equal(dev.level_perm(l), host.level_perm(l)), l
        if l < min(nagg, dev.num_levels - 1):
            m1, m2 = dev.level_agg_markers(l)
            h1, h2 = host.level_agg_markers(l)
            assert np.array_equal(m1, h1) and np.array_equal(m2, h2), l
            assert (m2 == 1).sum() < (m1 == 1).sum() < len(m1)


@pytest.mark.parametrize("kw", [dict(agg_num_levels=1), dict(agg_num_levels=2, agg_pmax_elmts=4),
                                dict(agg_num_levels=1, agg_pmax_elmts=4, agg_p12_max_elmts=4),
                                dict(agg_num_levels=2, agg_trunc_factor=0.2, agg_p12_trunc_factor=0.1)],
                         ids=lambda kw: "-".join("%s%s" % (k.replace("agg_", ""), v) for k, v in kw.items()))
@pytest.mark.parametrize("name", ["lap7_24", "lap27_16", "randmm"])
def test_device_levels_are_bit_identical_to_the_host_setup(mi, name, kw, monkeypatch):
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    monkeypatch.setenv("MI_HYPRE_LOCALITY_ORDER", "0")
    A, Ah = _pair(mi, name)
    dev = mi.BoomerAMG(print_level=0, keep_agg_markers=1, agg_interp_type=5, **kw)
    dev.setup(A)
    host = host_amg(mi, Ah, agg_interp_type=5, **kw)
    _assert_bit_identical(dev, host, kw["agg_num_levels"])


@pytest.mark.parametrize("name,kw", [("lap7_24", dict(agg_num_levels=1, agg_pmax_elmts=4)), ("randmm", dict(agg_num_levels=2))])
def test_device_levels_with_the_locality_numbering(mi, name, kw, monkeypatch):
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    monkeypatch.setenv("MI_HYPRE_LOCALITY_ORDER", "1")
    A, Ah = _pair(mi, name)
    dev = mi.BoomerAMG(print_level=0, keep_agg_markers=1, agg_interp_type=5, **kw)
    dev.setup(A)
    host = host_amg(mi, Ah, agg_interp_type=5, **kw)
    (applied, order), (happlied, horder) = dev.input_ordering(), host.input_ordering()
    assert applied and happlied and np.array_equal(order, horder)
    _assert_bit_identical(dev, host, kw["agg_num_levels"])


def test_other_coarsenings_keep_the_host_splitting_and_use_the_device_interpolation(mi, monkeypatch):
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    monkeypatch.setenv("MI_HYPRE_LOCALITY_ORDER", "0")
    A, Ah = _pair(mi, "lap7_24")
    kw = dict(agg_num_levels=1, agg_interp_type=5, coarsen_type=10, agg_pmax_elmts=4)
    dev = mi.BoomerAMG(print_level=0, keep_agg_markers=1, **kw)
    dev.setup(A)
    _assert_bit_identical(dev, host_amg(mi, Ah, **kw), 1)


def test_two_device_setups_are_bit_identical(mi, monkeypatch):
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    monkeypatch.setenv("MI_HYPRE_LOCALITY_ORDER", "0")
    A, _ = _pair(mi, "lap27_16")
    kw = dict(print_level=0, keep_agg_markers=1, agg_num_levels=2, agg_interp_type=5, agg_pmax_elmts=4, agg_p12_max_elmts=6)
    a1, a2 = mi.BoomerAMG(**kw), mi.BoomerAMG(**kw)
    a1.setup(A)
    a2.setup(A)
    _assert_bit_identical(a1, a2, 2)


def test_zero_denominator_fails_the_device_setup_like_the_host_setup(mi, monkeypatch):
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
        amg = mi.BoomerAMG(print_level=0, agg_num_levels=1, agg_interp_type=5)
        with pytest.raises(mi.HypreError, match=r"level 0: row \d+ has a zero denominator") as e:
            setup(amg)
        msgs.append(re.search(r"row \d+", str(e.value)).group(0))
        mi.call("HYPRE_ClearAllErrors")
    assert msgs[0] == msgs[1], msgs


def test_nothing_reads_memory_it_has_not_written():
    """MI_HYPRE_POISON_ALLOC=1 hands out every device block full of 0xFF bytes: two aggressive levels built on the
    device with both truncations (tests/agg2s_env_worker.py) give the same hierarchy, bit for bit, as without -- and
    as the host-only setup, which the worker checks itself."""
    def run(**env):
        e = dict(os.environ, MI_HYPRE_DEVICE_SETUP_MIN_ROWS="0", MI_HYPRE_LOCALITY_ORDER="0", **env)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "agg2s_env_worker.py")], env=e,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-3000:]
        return [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]

    assert run(MI_HYPRE_POISON_ALLOC="1") == run()


def test_gmres_needs_no_more_iterations_than_with_multipass(mi):
    """32^3, one aggressive level, GMRES(50) to 1e-8: x* = 1, and the two-stage interpolation does not lose against
    multipass on the same splitting."""
    n = 32
    its = {}
    for t in (5, 4):
        A, b, x, rhs = mi.build_laplace_system(n, n, n, 7)
        amg = mi.BoomerAMG(print_level=0, agg_num_levels=1, agg_interp_type=t)
        gm = mi.GMRES(tolerance=1e-8, max_iterations=100, kspace=50, print_level=0)
        gm.set_precond(amg)
        gm.setup(A, b, x)
        assert gm.solve(A, b, x) == 0
        assert gm.final_rel_res < 1e-8 and np.abs(x.get() - 1.0).max() < 1e-6, (t, gm.final_rel_res)
        its[t] = gm.num_iterations
        print("agg_interp_type %d: %d iterations, operator complexity %.3f" % (t, gm.num_iterations, amg.operator_complexity))
    assert its[5] <= its[4], its


def test_driver_runs_agg_interp_type_5(tmp_path):
    from tests.test_gpu_app import _run

    out = _run(tmp_path, """
linear_system:
  type: laplace_3d
  nx: 24
  ny: 24
  nz: 24
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
  agg_num_levels: 1
  agg_interp_type: 5
  agg_pmax_elmts: 4
  agg_p12_max_elmts: 6
  agg_p12_trunc_factor: 0.05
""")
    assert "not implemented" not in out and "NOT implemented" not in out, out[-2000:]
    m = re.search(r"max \|x - 1\| = ([0-9.eE+-]+)", out)
    assert m and float(m.group(1)) < 1e-6, out[-2000:]


def test_two_ranks_sharing_the_gpu_over_tcp_agree_with_one_rank():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MI_HYPRE_HOST_THREADS="2", OMP_NUM_THREADS="1",
               MI_HYPRE_LOCALITY_ORDER="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "30951", WORKER, "--mode", "solve", "--grid", "16", "--agg", "1", "--transport", "tcp"]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    assert p.stdout.count("agg2s rank ok") == 2, p.stdout[-4000:]
