"""GPU: update rounds of an assembled IJ matrix (set / add / constant values after HYPRE_IJMatrixAssemble) through
device pointers (kernels: csrc/ij_assembly.hip) and through numpy arrays (host path: parcsr.cpp).  The reference
everywhere is a FRESH matrix, host-assembled from all batches of all rounds concatenated, compared bit for bit: the host
blocks, the diag block read back from the device solve format, the column map and a product with a seeded vector
(tests/ij_cases.py: snapshot).  The CPU statement of the semantics: tests/test_ij_update_spec.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ij_cases as cases
from tests import ij_update_cases as upd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "ij_update_env_worker.py")
DIST_WORKER = os.path.join(ROOT, "tests", "ij_update_dist_worker.py")


def _fresh(mi, n, rounds, pairs=None):
    """the oracle: one host assembly of everything"""
    A = cases.new_matrix(mi, 0, n - 1)
    cases.stage(mi, A, upd.oracle_batches(rounds, pairs), device=False)
    A.assemble()
    snap = cases.snapshot(mi, A)
    A.destroy()
    return snap


def _updated(mi, n, rounds, device, first_device=True):
    """rounds[0] assembled, the others applied as update rounds through device pointers or numpy arrays"""
    A = cases.new_matrix(mi, 0, n - 1)
    cases.stage(mi, A, rounds[0], first_device)
    A.assemble()
    for ops in rounds[1:]:
        c0, d0 = mi.counter("ij_value_updates"), mi.counter("ij_device_value_updates")
        upd.apply_round(mi, A, ops, device=device)
        assert mi.counter("ij_value_updates") - c0 == 1
        assert mi.counter("ij_device_value_updates") - d0 == (1 if device else 0)
    snap = cases.snapshot(mi, A)
    A.destroy()
    return snap


def _check(mi, n, rounds, pairs=None):
    ref = _fresh(mi, n, rounds, pairs)
    assert cases.same(_updated(mi, n, rounds, True), ref)
    assert cases.same(_updated(mi, n, rounds, False), ref)
    return ref


@pytest.fixture(scope="module")
def lap(mi):
    return {(12, 7): cases.laplace_triples(mi, 12, 7), (10, 27): cases.laplace_triples(mi, 10, 27)}


def _forms(r, c, v, add, form, seed):
    if form == "row_order":  # the boundary-detection shortcut: no sort
        return [(r.copy(), c.copy(), v.copy(), add)]
    if form == "shuffled":
        p = np.random.default_rng(seed).permutation(len(v))
        return [(r[p].copy(), c[p].copy(), v[p].copy(), add)]
    cut = [0, 1001, 5003, len(v)]  # a row continues in the next batch
    return [(r[a:b].copy(), c[a:b].copy(), v[a:b].copy(), add) for a, b in zip(cut[:-1], cut[1:])]


@pytest.mark.parametrize("form", ["row_order", "shuffled", "three_batches"])
@pytest.mark.parametrize("n,stencil", [(12, 7), (10, 27)])
def test_device_round_equals_host_round_equals_fresh_assembly(mi, lap, n, stencil, form):
    r, c, v = lap[(n, stencil)]
    rng = np.random.default_rng(n + stencil)
    v2 = 1.5 * v + rng.standard_normal(len(v))
    v3 = rng.choice([cases.BIG, 1.0, -cases.BIG, 0.5], size=len(v))
    rounds = [[(r, c, v, False)], _forms(r, c, v2, False, form, 5), _forms(r, c, v3, True, form, 6)]
    _check(mi, n ** 3, rounds)


def test_duplicates_small(mi):
    n, pairs, rounds = upd.small_rounds()
    ref = _check(mi, n, rounds)
    (dia, dja, da), _ = cases.fold([b for ops in rounds for b in ops], 0, n - 1, 0, n - 1)
    assert np.array_equal(ref["ia0"], dia) and np.array_equal(ref["ja0"], dja) and np.array_equal(ref["a0"], da.view(np.int64))


def test_duplicates_large(mi):
    n, first = cases.duplicates_large()
    rng = np.random.default_rng(99)
    second = [(r.copy(), c.copy(), rng.permutation(v), add) for r, c, v, add in first]
    _check(mi, n, [first, [second[1], second[0], second[2]]])


def test_constants_on_the_device_path(mi, lap):
    """SetConstantValues(0) then Adds, a constant between two Add batches, a constant as the last call"""
    n, pairs, rounds = upd.small_rounds()
    adds = [b for b in rounds[1] if b[3]]
    _check(mi, n, [rounds[0], [("const", 0.0)] + adds, [adds[0], ("const", 2.5), adds[1], rounds[1][1]],
                   [adds[1], ("const", -1.0)], [adds[0]]], pairs)


def _threshold_operator(mi):
    """the operator of test_gpu_ij_device_assembly.py::test_rows_at_the_sort_thresholds"""
    cap = mi.counter("ij_device_sort_lds_capacity")
    rng = np.random.default_rng(23)
    lens = [2, 63, 64, 65, 255, 256, 257, cap - 1, cap, cap + 1, 1500, 3000]
    rows, cols = [], []
    for i, L in enumerate(lens):
        rows.append(np.full(L, 10 * i + 1, dtype=np.int64))
        cols.append(rng.integers(0, max(2, (2 * L) // 3), size=L).astype(np.int64))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = rng.choice([cases.BIG, 1.0, -cases.BIG, 0.25], size=len(rows))
    h = len(rows) // 3
    p = rng.permutation(len(rows))
    rows, cols, vals = rows[p], cols[p], vals[p]
    return 3000, [(rows[:h].copy(), cols[:h].copy(), vals[:h].copy(), True), (rows[h:].copy(), cols[h:].copy(), vals[h:].copy(), True)]


@pytest.mark.parametrize("which", ["all_entries", "first_and_last"])
def test_row_lengths_where_the_kernels_change(mi, which):
    n, first = _threshold_operator(mi)
    pairs = np.array(upd.pattern_of(first), dtype=np.int64)
    rng = np.random.default_rng(31)
    if which == "first_and_last":
        keep = np.r_[True, pairs[1:, 0] != pairs[:-1, 0]] | np.r_[pairs[1:, 0] != pairs[:-1, 0], True]
        pairs = pairs[keep]
    rep = np.repeat(np.arange(len(pairs)), rng.integers(1, 5, size=len(pairs)))  # 1-4 operations per stored entry
    rep = rep[rng.permutation(len(rep))]
    vals = rng.choice([cases.BIG, 1.0, -cases.BIG, 0.25, 3.0], size=len(rep))
    to = rng.integers(0, 3, size=len(rep))
    second = [(pairs[rep[to == b], 0].copy(), pairs[rep[to == b], 1].copy(), vals[to == b].copy(), add)
              for b, add in enumerate((True, False, True))]
    _check(mi, n, [first, second])


def test_partial_round_leaves_every_other_value_alone(mi, lap):
    r, c, v = lap[(12, 7)]
    n = 12 ** 3
    rng = np.random.default_rng(8)
    rows = rng.choice(n, size=n // 10, replace=False)
    m = np.isin(r, rows)
    p = rng.permutation(int(m.sum()))
    second = [(r[m][p].copy(), c[m][p].copy(), rng.standard_normal(int(m.sum())), True)]
    ref = _check(mi, n, [[(r, c, v, False)], second])
    base = _fresh(mi, n, [[(r, c, v, False)]])
    touched = np.repeat(np.isin(np.arange(n), rows), np.diff(base["ia0"]))
    assert np.array_equal(ref["a0"][~touched], base["a0"][~touched]) and (ref["a0"][touched] != base["a0"][touched]).all()


def test_value_dictionary_comes_and_goes(mi):
    """22^3 7-point: the smallest cube whose diag block (71 632 entries) is large enough for a value dictionary"""
    import scipy.sparse as sp

    n = 22 ** 3
    r, c, v = cases.laplace_triples(mi, 22, 7)
    rng = np.random.default_rng(17)
    many = rng.standard_normal(len(v))
    two = np.where(r == c, 8.0, -1.25)
    A = cases.new_matrix(mi, 0, n - 1)
    cases.stage(mi, A, [(r, c, v, False)], True)
    A.assemble()
    assert mi.parcsr_value_kind(A) == 8
    xv = np.random.default_rng(3).standard_normal(n)  # the vector of cases.snapshot
    for vals, kind in ((many, 0), (two, 8), (many, 0)):
        upd.apply_round(mi, A, [(r, c, vals, False)], device=True)
        assert mi.parcsr_value_kind(A) == kind
        snap = cases.snapshot(mi, A)
        assert cases.same(snap, _fresh(mi, n, [[(r, c, vals, False)]]))
        y = sp.csr_matrix((vals, (r, c)), shape=(n, n)) @ xv
        assert np.abs(snap["matvec"].view(np.float64) - y).max() <= 1e-13 * np.abs(y).max()
    A.destroy()


@pytest.mark.parametrize("where", ["diag", "halo_range"])
def test_refusal_on_the_device_path(mi, lap, where):
    r, c, v = lap[(12, 7)]
    n = 12 ** 3
    A = cases.new_matrix(mi, 0, n - 1)
    cases.stage(mi, A, [(r, c, v, False)], True)
    A.assemble()
    before, stamp = cases.snapshot(mi, A), mi.assembly_stamp(A)
    br, bc = (5, 900) if where == "diag" else (7, n + 3)
    p = np.random.default_rng(2).permutation(len(v))
    bad = (np.r_[r[p][:500], br, r[p][500:], 9], np.r_[c[p][:500], bc, c[p][500:], 1500], np.r_[2 * v[p][:500], 1.0, 2 * v[p][500:], 1.0], False)
    c0, d0 = mi.counter("ij_value_updates"), mi.counter("ij_device_value_updates")
    with pytest.raises(mi.HypreError) as e:
        upd.apply_round(mi, A, [("const", 3.0), (r, c, 2 * v, True), bad], device=True)
    assert f"row {br}," in str(e.value) and f"column {bc})" in str(e.value) and "HYPRE_IJMatrixAssemble returned 1:" in str(e.value)
    mi.call("HYPRE_ClearAllErrors")
    assert cases.same(cases.snapshot(mi, A), before) and mi.assembly_stamp(A) == stamp
    assert (mi.counter("ij_value_updates"), mi.counter("ij_device_value_updates")) == (c0, d0)
    upd.apply_round(mi, A, [(r, c, 2 * v, True)], device=True)
    assert cases.same(cases.snapshot(mi, A), _fresh(mi, n, [[(r, c, v, False)], [(r, c, 2 * v, True)]]))
    assert mi.assembly_stamp(A) != stamp
    A.destroy()


def test_a_row_of_another_rank_is_refused_on_the_device_path(mi, lap):
    r, c, v = lap[(12, 7)]
    n = 12 ** 3
    A = cases.new_matrix(mi, 0, n - 1)
    cases.stage(mi, A, [(r, c, v, False)], True)
    A.assemble()
    before = cases.snapshot(mi, A)
    with pytest.raises(mi.HypreError) as e:
        upd.apply_round(mi, A, [(np.r_[r[:10], n + 4], np.r_[c[:10], 3], np.r_[v[:10], 1.0], True)], device=True)
    assert f"row {n + 4}," in str(e.value) and "column 3)" in str(e.value)
    mi.call("HYPRE_ClearAllErrors")
    assert cases.same(cases.snapshot(mi, A), before)
    A.destroy()


def test_mixed_round_is_demoted_to_the_host(mi, lap):
    r, c, v = lap[(12, 7)]
    n = 12 ** 3
    h = len(v) // 2
    A = cases.new_matrix(mi, 0, n - 1)
    cases.stage(mi, A, [(r, c, v, False)], True)
    A.assemble()
    d0 = mi.counter("ij_device_value_updates")
    cases.stage(mi, A, [(r[:h + 7].copy(), c[:h + 7].copy(), 2 * v[:h + 7], True)], True)
    A.set_constant_values(0.5)
    cases.stage(mi, A, [(r[h:].copy(), c[h:].copy(), 3 * v[h:], True)], False)
    A.assemble()
    assert mi.counter("ij_device_value_updates") == d0
    ref = _fresh(mi, n, [[(r, c, v, False)], [("const", 0.5), (r[h:], c[h:], 3 * v[h:], True)]], list(zip(r.tolist(), c.tolist())))
    assert cases.same(cases.snapshot(mi, A), ref)
    A.destroy()


def test_aliased_level_zero_asks_for_setup_again(mi):
    """a diagonal matrix gives a one-level hierarchy whose level 0 is the caller's matrix itself"""
    n = 50
    idx = np.arange(n, dtype=np.int64)
    d1 = 1.0 + np.arange(n) / 7.0
    A = cases.new_matrix(mi, 0, n - 1)
    cases.stage(mi, A, [(idx, idx, d1, False)], True)
    A.assemble()
    bv = np.cos(idx.astype(np.float64))
    b, x = mi.IJVector(0, n - 1, bv), mi.IJVector(0, n - 1, np.zeros(n))
    amg = mi.BoomerAMG(print_level=0)
    amg.setup(A)
    assert amg.num_levels == 1
    amg.solve(A, b, x)
    upd.apply_round(mi, A, [(idx, idx, 3.0 * d1 + 0.5, False)], device=True)
    with pytest.raises(mi.HypreError) as e:
        amg.solve(A, b, x)
    assert "Setup again" in str(e.value) and "returned 1:" in str(e.value)
    mi.call("HYPRE_ClearAllErrors")
    amg.setup(A)
    x.set(np.zeros(n))
    amg.solve(A, b, x)
    assert np.abs(x.get() - bv / (3.0 * d1 + 0.5)).max() <= 4 * np.finfo(np.float64).eps * np.abs(bv / (3.0 * d1 + 0.5)).max()


def _child(args, env=None, timeout=300):
    e = dict(os.environ, **{k: str(v) for k, v in (env or {}).items()})
    p = subprocess.run([sys.executable, WORKER] + args, env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-4000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


@pytest.mark.parametrize("locality", [0, 1])
def test_stale_preconditioner_then_setup_again(locality):
    """GMRES(20) + BoomerAMG set up on A1 = convection_diffusion_3d(12), the matrix updated to A2 = 3 A1 + diag(seeded
    values in [0, 1]).  Without a new Setup the hierarchy (it owns a renumbered copy of level 0) preconditions the OLD
    operator while the Krylov matvec uses the new one: the solve converges to A2's solution -- true relative residual
    (scipy, A2) <= 1e-8 for a solver tolerance of 1e-9; the factor 10 covers the gap between the recursive estimate
    and the recomputed residual.  Setup again on the same handles: every level's operators equal, bit for bit, those of
    fresh handles on a fresh A2, and the iteration counts are equal."""
    r = _child(["stale"], dict(MI_HYPRE_LOCALITY_ORDER=locality))
    print(r)
    assert r["stale_true_rel_res"] <= 1e-8 and r["stale_iters"] >= 2
    assert r["levels"] >= 2 and r["levels_equal"] and r["resetup_iters"] == r["fresh_iters"] and r["x_equal"]


def test_poisoned_allocations_give_the_same_bits():
    a = _child(["round"], dict(MI_HYPRE_LOCALITY_ORDER=0))
    b = _child(["round"], dict(MI_HYPRE_LOCALITY_ORDER=0, MI_HYPRE_POISON_ALLOC=1))
    assert a["digest"] == b["digest"] and a["iters"] == b["iters"] and a["device_value_updates"] == b["device_value_updates"] == 1


@pytest.mark.parametrize("nproc,mode", [(2, "slabs"), (3, "empty")])
def test_update_rounds_on_ranks_that_share_the_gpu(nproc, mode):
    """2 ranks, and 3 ranks of which one owns no rows; every rank runs under the spawner's time limit"""
    from tests.test_dist import _spawn_direct

    env = dict(os.environ, MI_HYPRE_LOCALITY_ORDER="0")
    out = _spawn_direct([DIST_WORKER, mode], nproc, 29930 + nproc, env, 240)
    assert out.count("ij update rank ok") == nproc, out[-4000:]
