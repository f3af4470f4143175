"""GPU: IJ matrices whose entries arrive in device memory are assembled on the device (csrc/ij_assembly.hip).  The
reference in every case is the same entries given as numpy arrays -- the host assembly, whose semantics
tests/test_ij_assembly_spec.py pins -- and the comparison is bit for bit: the host blocks, the diag block read back from
the device solve format, the column map, and a product with a seeded vector.  Device arrays are torch CUDA tensors
passed by address."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ij_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "ij_env_worker.py")
DIST_WORKER = os.path.join(ROOT, "tests", "ij_device_dist_worker.py")


def _both(mi, n, batches, **kw):
    """(device-assembled snapshot, host-assembled snapshot) of the same batches on an n x n matrix"""
    snaps = []
    for device in (True, False):
        before = mi.counter("ij_device_assemblies")
        A = cases.new_matrix(mi, 0, n - 1, **kw)
        cases.stage(mi, A, batches, device)
        A.assemble()
        assert mi.counter("ij_device_assemblies") - before == (1 if device else 0)
        snaps.append(cases.snapshot(mi, A))
        A.destroy()
    return snaps


def _shuffled(triples, seed):
    p = np.random.default_rng(seed).permutation(len(triples[0]))
    return tuple(np.ascontiguousarray(t[p]) for t in triples)


@pytest.fixture(scope="module")
def lap(mi):
    return {(12, 7): cases.laplace_triples(mi, 12, 7), (10, 27): cases.laplace_triples(mi, 10, 27)}


@pytest.mark.parametrize("n,stencil", [(12, 7), (10, 27)])
def test_row_order(mi, lap, n, stencil):
    r, c, v = lap[(n, stencil)]
    dev, host = _both(mi, n ** 3, [(r, c, v, False)])
    assert cases.same(dev, host) and dev["ia0"][-1] == len(v)


@pytest.mark.parametrize("n,stencil", [(12, 7), (10, 27)])
def test_shuffled(mi, lap, n, stencil):
    r, c, v = _shuffled(lap[(n, stencil)], 5)
    dev, host = _both(mi, n ** 3, [(r, c, v, False)])
    assert cases.same(dev, host)


def test_row_order_across_batches(mi, lap):
    """row order kept across three batches, a row continuing in the next batch: the boundary-detection path"""
    r, c, v = lap[(12, 7)]
    cut = [0, 1001, 5003, len(v)]
    batches = [(r[a:b].copy(), c[a:b].copy(), v[a:b].copy(), False) for a, b in zip(cut[:-1], cut[1:])]
    dev, host = _both(mi, 12 ** 3, batches)
    assert cases.same(dev, host)


@pytest.mark.parametrize("case", ["small", "large"])
def test_duplicates(mi, case):
    n, batches = cases.duplicates_small() if case == "small" else cases.duplicates_large()
    dev, host = _both(mi, n, batches)
    assert cases.same(dev, host)
    if case == "small":  # and both are the specification
        (dia, dja, da), _ = cases.fold(batches, 0, n - 1, 0, n - 1)
        assert np.array_equal(dev["ia0"], dia) and np.array_equal(dev["ja0"], dja)
        assert np.array_equal(dev["a0"], da.view(np.int64))


def test_ragged_rows_beyond_the_lds_sort(mi):
    cap = mi.counter("ij_device_sort_lds_capacity")
    n, batches = cases.ragged(long_len=10000)
    assert 0 < cap < 10000  # the long row takes the any-length path
    dev, host = _both(mi, n, batches)
    assert cases.same(dev, host)
    lens = np.diff(dev["ia0"])
    long_cols = np.concatenate([b[1][b[0] == 5000] for b in batches])
    assert len(long_cols) == 10000 and lens[5000] == len(np.unique(long_cols)) < 10000
    assert (lens == 0).sum() > 10000 and (lens == 1).sum() > 1000


def test_rows_at_the_sort_thresholds(mi):
    """one unsorted row with duplicates at every length where the per-row sort changes its kernel"""
    cap = mi.counter("ij_device_sort_lds_capacity")
    rng = np.random.default_rng(23)
    lens = [2, 63, 64, 65, 255, 256, 257, cap - 1, cap, cap + 1, 1500, 3000]  # several rows on the any-length path
    n = 3000
    rows, cols = [], []
    for i, L in enumerate(lens):
        rows.append(np.full(L, 10 * i + 1, dtype=np.int64))
        cols.append(rng.integers(0, max(2, (2 * L) // 3), size=L).astype(np.int64))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = rng.choice([cases.BIG, 1.0, -cases.BIG, 0.25], size=len(rows))
    h = len(rows) // 3
    p = rng.permutation(len(rows))
    rows, cols, vals = rows[p], cols[p], vals[p]
    batches = [(rows[:h].copy(), cols[:h].copy(), vals[:h].copy(), True), (rows[h:].copy(), cols[h:].copy(), vals[h:].copy(), True)]
    dev, host = _both(mi, n, batches)
    assert cases.same(dev, host)


def test_ncols_form_with_gaps(mi):
    import torch

    rng = np.random.default_rng(4)
    n = 300
    sel = np.sort(rng.choice(n, size=120, replace=False)).astype(np.int64)
    sel = sel[rng.permutation(len(sel))]
    ncols = rng.integers(0, 9, size=len(sel)).astype(np.int32)
    gaps = rng.integers(0, 4, size=len(sel))
    row_indexes = (np.cumsum(ncols + gaps) - ncols - gaps + gaps).astype(np.int32)  # start of row i, gaps before each row
    span = int(row_indexes[-1] + ncols[-1]) + 3
    cols = rng.integers(0, n, size=span).astype(np.int64)
    vals = rng.standard_normal(span)
    snaps = []
    for device in (True, False):
        for packed in (False, True):
            A = cases.new_matrix(mi, 0, n - 1)
            if packed:  # row_indexes == NULL: the rows follow each other
                tot = int(ncols.sum())
                arrs = [ncols, sel, None, cols[:tot].copy(), vals[:tot].copy()]
            else:
                arrs = [ncols, sel, row_indexes, cols, vals]
            if device:
                t = [None if a is None else torch.from_numpy(a).cuda() for a in arrs]
                torch.cuda.synchronize()
                ptr = [0 if x is None else x.data_ptr() for x in t]
            else:
                ptr = [0 if a is None else a.ctypes.data for a in arrs]
            before = mi.counter("ij_entries_fetched_to_host")
            A.set_values_rows_ptr(len(sel), ptr[0], ptr[1], ptr[2], ptr[3], ptr[4])
            A.set_values_rows_ptr(len(sel), ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], add=True)
            assert mi.counter("ij_entries_fetched_to_host") == before
            A.assemble()
            snaps.append(cases.snapshot(mi, A))
            A.destroy()
    assert cases.same(snaps[0], snaps[2]) and cases.same(snaps[1], snaps[3])
    assert snaps[0]["ia0"][-1] > 300


def test_set_constant_values_and_overwritten_inputs(mi, lap):
    import torch

    r, c, v = _shuffled(lap[(12, 7)], 9)
    n = 12 ** 3
    # (f) constant values between SetValues and Assemble
    snaps = []
    for device in (True, False):
        A = cases.new_matrix(mi, 0, n - 1)
        cases.stage(mi, A, [(r, c, v, False)], device)
        mi.call("HYPRE_IJMatrixSetConstantValues", A.h, 0.375)
        A.assemble()
        snaps.append(cases.snapshot(mi, A))
        A.destroy()
    assert cases.same(*snaps) and set(np.unique(snaps[0]["a0"].view(np.float64))) == {0.375}
    # (g) the caller overwrites its arrays after SetValues
    keep = []
    A = cases.new_matrix(mi, 0, n - 1)
    cases.stage(mi, A, [(r, c, v, False)], True, keep=keep)
    for t in keep[0]:
        t.fill_(float("nan") if t.dtype == torch.float64 else -1)
    torch.cuda.synchronize()
    A.assemble()
    dev = cases.snapshot(mi, A)
    A.destroy()
    B = cases.new_matrix(mi, 0, n - 1)
    cases.stage(mi, B, [(r, c, v, False)], False)
    B.assemble()
    assert cases.same(dev, cases.snapshot(mi, B))


def test_two_assemblies_are_bit_identical(mi, lap):
    r, c, v = _shuffled(lap[(10, 27)], 5)
    dup = (np.concatenate([r, r[:5000]]), np.concatenate([c, c[:5000]]), np.concatenate([v, v[:5000]]))
    snaps = []
    for _ in range(2):
        A = cases.new_matrix(mi, 0, 999)
        cases.stage(mi, A, [dup + (True,)], True)
        A.assemble()
        snaps.append(cases.snapshot(mi, A))
        A.destroy()
    assert cases.same(*snaps)


def test_counters(mi, lap):
    """device-pointer batches are assembled on the device and nothing of them is fetched; numpy batches and a mix of
    the two take the host path"""
    import torch

    r, c, v = lap[(12, 7)]
    n = 12 ** 3
    asm, fetched = mi.counter("ij_device_assemblies"), mi.counter("ij_entries_fetched_to_host")
    mirror = mi.counter("ij_host_mirror_bytes")
    A = cases.new_matrix(mi, 0, n - 1)
    cases.stage(mi, A, [(r, c, v, False)], True)
    A.assemble()
    assert mi.counter("ij_device_assemblies") == asm + 1
    assert mi.counter("ij_entries_fetched_to_host") == fetched
    assert mi.counter("ij_host_mirror_bytes") - mirror == 8 * (n + 1) * 2 + 12 * len(v)
    B = cases.new_matrix(mi, 0, n - 1)
    cases.stage(mi, B, [(r, c, v, False)], False)
    B.assemble()
    assert mi.counter("ij_device_assemblies") == asm + 1
    assert mi.counter("ij_entries_fetched_to_host") == fetched
    # mixed: a device batch, then a host batch -- the device batch is fetched, the host path assembles
    Cm = cases.new_matrix(mi, 0, n - 1)
    h = len(v) // 2
    cases.stage(mi, Cm, [(r[:h].copy(), c[:h].copy(), v[:h].copy(), False)], True)
    cases.stage(mi, Cm, [(r[h:].copy(), c[h:].copy(), v[h:].copy(), False)], False)
    t = [torch.from_numpy(x[:10].copy()).cuda() for x in (r, c, v)]
    torch.cuda.synchronize()
    Cm.set_values_ptr(10, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), add=True)  # a device batch after a host one
    Cm.assemble()
    assert mi.counter("ij_device_assemblies") == asm + 1
    assert mi.counter("ij_entries_fetched_to_host") == fetched + h + 10
    v2 = v.copy()
    v2[:10] *= 2
    assert cases.same(cases.snapshot(mi, Cm), _both(mi, n, [(r, c, v2, False)])[1])


def test_refusals(mi, lap):
    n, batches = cases.duplicates_small()
    bad_row = [(b[0].copy(), b[1], b[2], b[3]) for b in batches]
    bad_row[1][0][5] = 40
    bad_row[2][0][2] = 77
    bad_col = [(b[0], b[1].copy(), b[2], b[3]) for b in batches]
    bad_col[0][1][3] = 45
    msgs = {}
    for device in (True, False):
        for name, bb in (("row", bad_row), ("col", bad_col)):
            A = cases.new_matrix(mi, 0, n - 1)
            cases.stage(mi, A, bb, device)
            with pytest.raises(mi.HypreError) as e:
                A.assemble()
            msgs[(device, name)] = str(e.value)
            mi.call("HYPRE_ClearAllErrors")
            if device:  # a refused device assembly is final: no second attempt on consumed batches, no empty matrix
                with pytest.raises(mi.HypreError, match="earlier assembly of this matrix failed"):
                    A.assemble()
                mi.call("HYPRE_ClearAllErrors")
            A.destroy()
    assert "row 40 is not owned by this rank" in msgs[(True, "row")] and "row 40 is not owned" in msgs[(False, "row")]
    assert "columns outside the single rank's range" in msgs[(True, "col")]
    assert msgs[(True, "col")] == msgs[(False, "col")]
    dev, host = _both(mi, n, batches)  # the next assembly in the same process succeeds
    assert cases.same(dev, host)


def test_vector_device_indices(mi):
    import torch

    lo, hi = 100, 1099
    rng = np.random.default_rng(8)
    idx = (lo + rng.permutation(hi - lo + 1)[:700]).astype(np.int64)
    val = rng.standard_normal(len(idx))
    out = []
    for device in (True, False):
        v = mi.IJVector(lo, hi, np.full(hi - lo + 1, 2.0))
        before = mi.counter("ij_entries_fetched_to_host")
        if device:
            ti, tv = torch.from_numpy(idx).cuda(), torch.from_numpy(val).cuda()
            torch.cuda.synchronize()
            for fn in ("HYPRE_IJVectorSetValues", "HYPRE_IJVectorAddToValues"):
                mi.call(fn, v.h, len(idx), mi.vp(ti.data_ptr()), mi.vp(tv.data_ptr()))
            assert mi.counter("ij_entries_fetched_to_host") == before
            bad = torch.tensor([lo, hi + 1, lo - 5], dtype=torch.int64).cuda()
            torch.cuda.synchronize()
            with pytest.raises(mi.HypreError, match=f"index {hi + 1} outside the local range"):
                mi.call("HYPRE_IJVectorSetValues", v.h, 3, mi.vp(bad.data_ptr()), mi.vp(tv.data_ptr()))
            mi.call("HYPRE_ClearAllErrors")
        else:
            for fn in ("HYPRE_IJVectorSetValues", "HYPRE_IJVectorAddToValues"):
                mi.call(fn, v.h, len(idx), idx, val)
            with pytest.raises(mi.HypreError, match="outside the local range"):
                mi.call("HYPRE_IJVectorSetValues", v.h, 3, np.array([lo, hi + 1, lo - 5], dtype=np.int64), val)
            mi.call("HYPRE_ClearAllErrors")
        out.append(v.get().view(np.int64))
    assert np.array_equal(out[0], out[1])
    assert (out[0].view(np.float64) != 2.0).sum() == len(idx)


@pytest.mark.parametrize("n,stencil", [(9, 7), (7, 27)])
def test_device_generator_equals_host_generator(mi, n, stencil):
    import ctypes as C

    N = n ** 3
    ranges = [(0, N - 1)] + [mi.row_partition(N, 3, r) for r in (0, 1)]
    for lo, hi in ranges:
        r, c, v = cases.laplace_triples(mi, n, stencil, lo, hi)
        g = mi.laplace3d(n, n, n, stencil, lo, hi)
        rhs = np.ctypeslib.as_array(C.cast(g["rhs"], C.POINTER(mi.c_dbl)), shape=(g["nloc"],)).copy()
        mi.laplace3d_free(g)
        d = mi.laplace3d_device(n, n, n, stencil, lo, hi)
        assert d["nnz"] == len(v) and d["nloc"] == hi - lo + 1
        got = {}
        for k, dt, cnt in (("rows", np.int64, len(v)), ("cols", np.int64, len(v)), ("vals", np.float64, len(v)),
                           ("rhs", np.float64, hi - lo + 1)):
            got[k] = np.zeros(cnt, dtype=dt)
            mi.lib().hypre_Memcpy(got[k].ctypes.data, d[k], got[k].nbytes, 0, 1)
        mi.laplace3d_device_free(d)
        assert np.array_equal(got["rows"], r) and np.array_equal(got["cols"], c)
        assert np.array_equal(got["vals"].view(np.int64), v.view(np.int64))
        assert np.array_equal(got["rhs"].view(np.int64), rhs.view(np.int64))


def _solve(mi, n, device):
    N = n ** 3
    A = cases.new_matrix(mi, 0, N - 1)
    if device:
        g = mi.laplace3d_device(n, n, n, 7, 0, N - 1)
        A.set_values_ptr(g["nnz"], g["rows"], g["cols"], g["vals"])
        mi.laplace3d_device_free(g)  # staged: the caller's arrays may go
    else:
        cases.stage(mi, A, [cases.laplace_triples(mi, n, 7) + (False,)], False)
    A.assemble()
    b = mi.IJVector(0, N - 1, np.cos(np.arange(N, dtype=np.float64)))
    x = mi.IJVector(0, N - 1, np.zeros(N))
    amg = mi.BoomerAMG(print_level=0)
    gm = mi.GMRES(tolerance=1e-9, max_iterations=60, kspace=50, print_level=0)
    gm.set_precond(amg)
    gm.setup(A, b, x)
    assert gm.solve(A, b, x) == 0
    return gm.num_iterations, gm.residual_history().view(np.int64), x.get().view(np.int64)


def test_solve_on_a_device_assembled_system(mi):
    before = mi.counter("ij_device_assemblies")
    it_d, hist_d, x_d = _solve(mi, 16, True)
    assert mi.counter("ij_device_assemblies") == before + 1
    it_h, hist_h, x_h = _solve(mi, 16, False)
    assert it_d == it_h and 2 < it_d < 30
    assert np.array_equal(hist_d, hist_h) and np.array_equal(x_d, x_h)


@pytest.mark.parametrize("env", [dict(MI_HYPRE_DEVICE_FORMAT_MIN_NNZ=1),
                                 dict(MI_HYPRE_DEVICE_FORMAT_MIN_NNZ=1, MI_HYPRE_POISON_ALLOC=1),
                                 dict(MI_HYPRE_DEVICE_ASSEMBLY=0)])
def test_switches_in_a_child_process(env):
    """the shuffled assembly and the solve again with the solve format built on the device from the assembled block
    (what large systems do), with poisoned allocations, and with the path switched off"""
    e = dict(os.environ, MI_HYPRE_LOCALITY_ORDER="0", **{k: str(v) for k, v in env.items()})
    p = subprocess.run([sys.executable, WORKER], env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    r = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert r["shuffled_equal"] and r["solve_equal"] and r["iters"] > 2
    assert r["device_assemblies"] == (0 if env.get("MI_HYPRE_DEVICE_ASSEMBLY") == 0 else 2)
    assert r["fetched"] == (0 if r["device_assemblies"] else r["entries"])


@pytest.mark.parametrize("nproc", [2, 3])
def test_device_assembly_on_ranks_that_share_the_gpu(nproc):
    from tests.test_dist import _spawn_direct

    env = dict(os.environ, MI_HYPRE_LOCALITY_ORDER="0")
    out = _spawn_direct([DIST_WORKER], nproc, 29870 + nproc, env, 300)
    assert out.count("ij device assembly rank ok") == nproc, out[-4000:]
