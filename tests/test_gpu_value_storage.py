"""GPU: fp32 value storage of the coarse-level AMG operators (HYPRE_MI_BoomerAMGSetValueStorage).

Mode 1 (fp32 stream) against mode 2 (fp64 stream of the fp32-rounded values), bit for bit, through relaxation passes,
C/F pairs, smoother steps and whole cycles of every level, with the library's switches set so that each kernel class
meets a narrowed operator; device setup against host-only setup; Krylov solves against mode 0; poisoned allocations; two
ranks.  The per-process work is in tests/value_storage_worker.py, whose assertions are the checks."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "value_storage_worker.py")
DIST_WORKER = os.path.join(ROOT, "tests", "value_storage_dist_worker.py")

pytestmark = pytest.mark.gpu


def _run(*args, **env):
    e = dict(os.environ, MI_HYPRE_LOCALITY_ORDER="0", **{k: str(v) for k, v in env.items()})
    p = subprocess.run([sys.executable, WORKER] + [str(a) for a in args], env=e, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def _has(r, *needles):
    return all(any(n in k for k in r["kernels"]) for n in needles), r["kernels"]


def test_tile_kernels_256_device_setup_row_mapped_R():
    """24^3 7-point, every level built on the device (R row-mapped): the 256-wide tile kernels, all SpMV epilogues"""
    r = _run("parity", "lap7", 24, MI_HYPRE_DEVICE_SETUP_MIN_ROWS=0, MI_HYPRE_NATURAL_R_MIN_NNZ=0)
    ok, names = _has(r, "gs_tile_k<false, 256, true>", "spmv_stream_xc<0, 0, false, 256, true>",
                     "spmv_stream_xc<1, 0, false, 256, true>")
    assert ok, names
    assert 1 in r["kinds"][1].values()
    assert r["row_mapped_R"] > 0  # restriction operators stored through a row map were among the narrowed ones


def test_tile_kernels_512():
    """16^3 27-point with the wide-tile threshold lowered: the 512-wide instantiations"""
    r = _run("parity", "lap27", 16, "types=6,8,13,18,11", MI_HYPRE_WIDE_TILE_MIN_ROWLEN=20)
    ok, names = _has(r, "gs_tile_k<false, 512, true>", "spmv_stream_xc<0, 0, false, 512, true>",
                     "spmv_stream_xc<1, 0, false, 512, true>")
    assert ok, names


def test_chunk_kernels():
    """the tile Gauss-Seidel kernel off: gs_dense_k on the 7-point hierarchy (15 to 30 entries in a coarse row), gs_group_k
    on a 1D chain (three).  The fp64 instantiations record names of the same form (gs_dense_k<16, 1>), and the worker reads
    classes that the mode-0 and mode-2 hierarchies wrote last, so only a name that ends in `, float>` shows that a float
    kernel ran."""
    r = _run("parity", "lap7", 20, "types=3,4,6,8,13,14", MI_HYPRE_GS_TILE=0)
    names = r["kernels"]
    assert any(k.startswith("gs_dense_k<") and k.endswith(", float>") for k in names), names
    assert not any("gs_tile_k" in k for k in names), names
    r = _run("parity", "chain", 3000, "types=3,4,6,8,13,14", MI_HYPRE_GS_TILE=0)
    ok, names = _has(r, "gs_group_k<8, 1, float>")
    assert ok and not any("gs_tile_k" in k for k in names), names


def test_plain_row_block_spmv():
    """no x cache anywhere: spmv_stream with both epilogues and the chunk Gauss-Seidel kernels on plain CSR"""
    r = _run("parity", "lap7", 16, "types=6,8,7,18,11,12", MI_HYPRE_XCACHE_MIN=100000)
    ok, names = _has(r, "spmv_stream<0, 0, float>", "spmv_stream<1, 0, float>")
    assert ok and not any("_xc<" in k for k in names), names


def test_other_chunk_size():
    """HYPRE_MI_SetGSChunk(4): gs_hybrid_k"""
    r = _run("parity", "lap7", 16, "gs_chunk=4", "types=3,6,8,13,14")
    ok, names = _has(r, "gs_hybrid_k<float>")
    assert ok, names


@pytest.mark.parametrize("zero_skip", [0, 1, 2])
def test_zero_skip_modes(zero_skip):
    """(3 is the default of every other case)"""
    _run("parity", "lap7", 16, "zero_skip=%d" % zero_skip, "types=6,8,13,14")


def test_dense_tail_off_and_first_level_2():
    a = _run("parity", "lap7", 16, "types=8,13", MI_HYPRE_DENSE_TAIL_ROWS=0)
    b = _run("parity", "lap7", 16, "types=8,13")
    assert a["levels"] == b["levels"] and a["kinds"] == b["kinds"]
    r = _run("parity", "lap7", 16, "types=8,13", "first_level=2")
    assert set(r["kinds"][1].values()) <= {0, 8} and 1 in r["kinds"][2].values()


def test_row_longer_than_a_tile():
    r = _run("parity", "arrow", 24, "types=6,8,13,18,11")
    assert r["longest_row_l1"] > 2048, r["longest_row_l1"]


def test_random_mmatrix_and_ilu_smoother():
    _run("parity", "mm", 0)
    _run("parity", "lap7", 14, "types=8,13", "smooth_type=5", "smooth_num_levels=2")


def test_fsai_smoother_steps():
    """HYPRE_MI_BoomerAMGSmoothLevel with the FSAI smoother (smooth_type 4) on a narrowed level, zero guess on and off"""
    _run("parity", "lap7", 14, "types=8,13", "smooth_type=4", "smooth_num_levels=2")


@pytest.mark.parametrize("name,n", [("lap7", 24), ("lap27", 16), ("mm", 0)])
def test_krylov_solves_against_fp64_storage(name, n):
    """Mode 1 and mode 2: identical residual histories.  Against mode 0: at most one iteration more (a perturbation of
    2^-24 per entry moves a history by that relative order, so the count changes only where mode 0's history crosses the
    tolerance within that distance), and a true relative residual -- numpy, the caller's unrounded matrix -- no larger
    than the greater of the tolerance and 1.001 x what mode 0 leaves."""
    r = _run("solve", name, n)
    for kname, res in r.items():
        m0, m1, m2 = res["modes"]["0"], res["modes"]["1"], res["modes"]["2"]
        h0, h1 = [float.fromhex(h) for h in m0["hist"]], [float.fromhex(h) for h in m1["hist"]]
        k = min(len(h0), len(h1))
        drift = max(abs(a - b) / a for a, b in zip(h0[:k], h1[:k]) if a > 0)
        print("%s %s: iterations %d / %d / %d (modes 0 / 1 / 2), true residual %.3e / %.3e, largest relative "
              "difference of the histories %.2e" % (name, kname, m0["iters"], m1["iters"], m2["iters"], m0["true_res"],
                                                     m1["true_res"], drift))
        assert m0["rc"] == 0 and m1["rc"] == 0 and m2["rc"] == 0
        assert m1["hist"] == m2["hist"] and m1["iters"] == m2["iters"], kname
        assert m1["iters"] <= m0["iters"] + 1, (kname, m1["iters"], m0["iters"])
        assert m1["true_res"] <= max(res["tol"], 1.001 * m0["true_res"]), (kname, m1["true_res"], m0["true_res"])


def test_nothing_reads_memory_it_has_not_written():
    """MI_HYPRE_POISON_ALLOC=1: every device block comes full of 0xFF bytes; the mode-1 setup, passes and cycle give the
    same bits as without"""
    a = _run("parity", "lap7", 16, "types=8,13", MI_HYPRE_POISON_ALLOC=1, MI_HYPRE_DEVICE_SETUP_MIN_ROWS=0)
    b = _run("parity", "lap7", 16, "types=8,13", MI_HYPRE_DEVICE_SETUP_MIN_ROWS=0)
    assert a["cycle"] == b["cycle"] and a["kinds"] == b["kinds"]


def test_two_ranks_sharing_the_gpu_over_tcp():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MI_HYPRE_HOST_THREADS="2", OMP_NUM_THREADS="1",
               MI_HYPRE_LOCALITY_ORDER="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "30961", DIST_WORKER, "--grid", "20"]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    assert p.stdout.count("value storage rank ok") == 2, p.stdout[-4000:]
