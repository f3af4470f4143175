"""GPU: the instantiation a launch records is the one the selection names (HYPRE_MI_SolveKernelChoice) for the
operator's descriptor, on the smallest operators that reach each branch of k::choose_stream_kernel and
k::choose_gs_kernel: one mat-vec under the level-0 class and one forward hybrid-GS pass of AMG level 0 per operator.

The descriptor is restated here from the operator's row pointers: x cache from a mean row length of 3, 4096-entry tiles
from a mean of 100, the 95th percentile of the row lengths, tiles made of whole 8-row chunks (dict_cases.tile_schedule)
that the tile Gauss-Seidel kernel sweeps where the mean row length exceeds 5 (MI_HYPRE_GS_TILE: 0 never, 1 always).  The
value format is what the library reports for the operator.  The mat-vec is held against scipy's float64 product by the
standard of test_gpu_kernels.test_spmv_vs_oracle: 1e-13 relative to the magnitude of the terms.

MI_HYPRE_GS_TILE is read once per process, so the case that needs the tile kernel off runs this file as a script in a
process of its own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)
from tests import dict_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu


def _lap5(n):
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n))
    return sp.kron(T, sp.identity(n)) + sp.kron(sp.identity(n), T)


def _band(n, half, constant):
    """n rows of 2 * half + 1 entries: the cyclic band; off-diagonals -1, or random in [-1.2, -0.8)"""
    rng = np.random.default_rng(n + half)
    i = np.repeat(np.arange(n), 2 * half)
    o = np.tile(np.r_[-half:0, 1:half + 1], n)
    v = np.full(len(i), -1.0) if constant else -rng.uniform(0.8, 1.2, len(i))
    d = 1.01 * np.bincount(i, weights=np.abs(v), minlength=n)
    return sp.coo_matrix((np.r_[v, d], (np.r_[i, np.arange(n)], np.r_[(i + o) % n, np.arange(n)])), shape=(n, n))


def operator(name):
    if name == "bidiagonal":
        M = sp.diags([-1.0, 2.0], [-1, 0], shape=(4099, 4099))
    elif name == "lap5-96":
        M = _lap5(96)
    elif name == "lap5-128":
        M = _lap5(128)
    elif name in ("band-constant", "band-random"):
        M = _band(704, 50, name == "band-constant")
    else:
        M = dc.relax_case(name)
    M = sp.csr_matrix(M)
    M.sort_indices()
    return M


# name -> (rows, entries, mat-vec kernel, sweep kernel): what the case is there to reach
CASES = {
    "bidiagonal": (4099, 8197, "spmv_stream<0, 1>", "gs_group_k<8, 1>"),
    "lap5-96": (9216, 45696, "spmv_stream_xc<0, 1, false, 256>", "gs_group_k<8, 1>"),
    "lap5-128": (16384, 81408, "spmv_stream_xc<0, 1, true, 256>", "gs_group_k<8, 1>"),
    "band-constant": (704, 71104, "spmv_stream_xc<0, 0, true, 512>", "gs_tile_k<true, 512>"),
    "band-random": (704, 71104, "spmv_stream_xc<0, 0, false, 512>", "gs_tile_k<false, 512>"),
}
TILES_OFF = "scattered"  # of dict_cases: about nine entries per row


def _tile_mode(avg):
    e = int(os.environ.get("MI_HYPRE_GS_TILE", -1))
    return e == 1 or (e != 0 and avg > 5.0)


def descriptor(indptr, shape, kind, chunk):
    """keyword arguments of mi.solve_kernel_choice for an operator with these row pointers and reported value kind"""
    ia = np.asarray(indptr, dtype=np.int64)
    n, nnz = len(ia) - 1, int(ia[-1])
    avg = nnz / n
    rb, tile, _ = dc.tile_schedule(ia)
    starts = rb[:-1]
    limit = np.minimum(n, (starts // 8192 + 1) * 8192)
    whole_chunks = bool(np.all(starts % 8 == 0) and np.all(ia[np.minimum(starts + 8, limit)] - ia[starts] <= tile - 1))
    xcache = avg >= 3.0
    return dict(xcache=xcache, tile_entries=tile, fp32=(kind == 1), dictionary=(kind == 8), chunk=chunk,
                tiles=xcache and shape[0] == shape[1] and whole_chunks and _tile_mode(avg), nnz=nnz, nrows=n,
                rowlen_p95=int(np.sort(np.diff(ia))[int((n - 1) * 0.95)]))


def run_case(mi, name):
    """(mat-vec kernel, sweep kernel) as the launches recorded them; asserts them against the selection's answer"""
    M = operator(name)
    n = M.shape[0]
    pids = (mi.PROF_SPMV_L0, mi.PROF_LVL_RELAX)
    for pid in pids:
        mi.profile_enable(pid, 8)
    try:
        chunk = mi.c_int()
        mi.call("HYPRE_MI_GetGSChunk", mi.C.byref(chunk))
        A = mi.matrix_from_scipy(M)
        rng = np.random.default_rng(n)
        xv = rng.standard_normal(n)
        x, y = mi.IJVector(0, n - 1, xv), mi.IJVector(0, n - 1, np.zeros(n))
        mi.call("HYPRE_ParCSRMatrixMatvec", 1.0, A.par, x.par, 0.0, y.par)
        spmv = mi.profile_kernel_name(mi.PROF_SPMV_L0)
        d = descriptor(M.indptr, M.shape, mi.parcsr_value_kind(A), chunk.value)
        want = mi.solve_kernel_choice(0, epilogue=0, level0=True, **d)
        print(f"{name}: {d}\n  mat-vec {spmv} (selection: {want})")
        assert spmv == want and spmv != ""
        assert np.all(np.abs(y.get() - M @ xv) <= 1e-13 * (abs(M) @ np.abs(xv) + 1.0))
        amg = mi.BoomerAMG(print_level=0)
        amg.setup(A)
        ia, ja, a, shape = amg.level_csr(0, 0)
        assert shape == M.shape and ia[-1] == M.nnz
        amg.relax_level(0, 3, 0, rng.standard_normal(n), rng.standard_normal(n))
        sweep = mi.profile_kernel_name(mi.PROF_LVL_RELAX)
        d = descriptor(ia, shape, amg.level_value_storage(0, 0)[0], chunk.value)
        want = mi.solve_kernel_choice(1, **d)
        print(f"  level 0: {d}\n  sweep {sweep} (selection: {want})")
        assert sweep == want and sweep != ""
        assert (amg.gs_sweep_paths(0, 0) is not None) == sweep.startswith("gs_tile_k")
        amg.destroy()
        A.destroy()
        return spmv, sweep
    finally:
        for pid in pids:
            mi.profile_enable(pid, 0)


@pytest.mark.parametrize("name", list(CASES))
def test_recorded_name_is_the_selected_one(mi, name):
    rows, entries, spmv, sweep = CASES[name]
    M = operator(name)
    assert M.shape == (rows, rows) and M.nnz == entries
    assert run_case(mi, name) == (spmv, sweep)


def test_dense_chunk_kernel_with_tiles_off():
    """mean row length between 8 and 16, MI_HYPRE_GS_TILE=0: gs_dense_k<16, .>, under its own name"""
    M = operator(TILES_OFF)
    assert 8.0 < M.nnz / M.shape[0] <= 16.0
    p = subprocess.run([sys.executable, os.path.abspath(__file__), TILES_OFF], env=dict(os.environ, MI_HYPRE_GS_TILE="0"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:]
    print(p.stdout)
    spmv, sweep = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert spmv == "spmv_stream_xc<0, 1, true, 256>"
    assert sweep in ("gs_dense_k<16, 1>", "gs_dense_k<16, 2>")


if __name__ == "__main__":
    import __graft_entry__ as ge

    binding = ge.load_binding()
    binding.init()
    print("RESULT " + json.dumps(run_case(binding, sys.argv[1])))
