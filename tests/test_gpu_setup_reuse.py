"""GPU: setup reuse (HYPRE_MI_BoomerAMGSetSetupReuse; DESIGN.md section 3, "Setup reuse").  The two kernels alone
through HYPRE_MI_CSRReuseOp against the restatement of tests/setup_reuse_ref.py, bit for bit; everything that is read
once per process in tests/setup_reuse_worker.py, a fresh child process per case with a time limit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from tests import setup_reuse_cases as rc
from tests import setup_reuse_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "setup_reuse_worker.py")


def _kernel_case():
    """A: 257 rows with 1 ... 9 entries; P: 257 x 61 with empty rows and unit rows, coarse column 7 shared by 200 fine
    rows (a long coarse row); the pattern of P^T A P"""
    rng = np.random.default_rng(20261019)
    n, nc = 257, 61
    rows, cols, vals = [], [], []
    for i in range(n):
        k = 1 + i % 9
        c = np.unique(np.concatenate([[i], rng.integers(0, n, size=k - 1)]))
        rows += [i] * len(c)
        cols += c.tolist()
        vals += rng.standard_normal(len(c)).tolist()
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    rows, cols, vals = [], [], []
    for i in range(n):
        if i % 17 == 3:
            continue  # an empty row
        if i % 5 == 0:
            c = np.array([i % nc])  # a unit row
            v = np.array([1.0])
        else:
            c = np.unique(rng.integers(0, nc, size=3))
            v = rng.uniform(0.1, 1.0, size=len(c))
        if i < 200 and 7 not in c and i % 17 != 3:
            c, v = np.append(c, 7), np.append(v, 0.25)
        rows += [i] * len(c)
        cols += c.tolist()
        vals += v.tolist()
    P = sp.csr_matrix((vals, (rows, cols)), shape=(n, nc))
    for M in (A, P):
        M.sort_indices()
    pat = (abs(P).T @ (abs(A) @ abs(P))).tocsr()
    pat.sort_indices()
    return A, P, pat


@pytest.mark.parametrize("lanes", [0, 1, 4, 16, 64])
def test_galerkin_values_kernel_has_the_bits_of_the_restatement(mi, lanes):
    """every lane count: a row longer than the lane group is walked in strides, so the long coarse row (more entries
    than 64 lanes at 1 and 4 lanes per row many times over) runs the kernel's only path for rows of any length"""
    A, P, pat = _kernel_case()
    assert np.diff(pat.indptr).max() > 48 and (P.getnnz(axis=0) >= 150).any()
    want, fits = ref.triple_product_into_pattern(A, P, pat)
    assert fits
    got = mi.csr_reuse_op(0, A, pat, P=P, lanes=lanes)
    assert rc.same_bits(got, want)
    C, B = ref.triple_product_scipy(A, P)
    assert (np.abs(C.data - got) <= 1e-13 * B.data).all()


def test_galerkin_values_kernel_small_empty_and_misfit(mi):
    one = sp.csr_matrix(np.array([[3.0]]))
    assert mi.csr_reuse_op(0, one, one, P=sp.csr_matrix(np.array([[0.5]])))[0] == 0.75
    # an empty product into an empty pattern
    A = sp.csr_matrix((np.array([2.0, 1.0]), (np.array([0, 1]), np.array([0, 1]))), shape=(2, 2))
    P = sp.csr_matrix((2, 1))
    assert len(mi.csr_reuse_op(0, A, sp.csr_matrix((1, 1)), P=P)) == 0
    # a pattern that lacks an entry of the product, and one with an entry the product lacks: the internal error, the
    # row, and nothing written
    A, P, pat = _kernel_case()
    short = pat.tolil()
    r = int(np.argmax(np.diff(pat.indptr)))
    short[r, pat.indices[pat.indptr[r]]] = 0
    short = short.tocsr()
    short.eliminate_zeros()
    full = sp.csr_matrix(np.ones(pat.shape))
    for bad, row in ((short, r), (full, None)):
        with pytest.raises(mi.HypreError) as e:
            mi.csr_reuse_op(0, A, bad, P=P)
        assert "internal error" in str(e.value) and "returned 1:" in str(e.value) and np.isnan(e.value.values).all()
        assert e.value.bad_row == row if row is not None else e.value.bad_row >= 0
        mi.call("HYPRE_ClearAllErrors")


def test_value_lookup_kernel(mi):
    A, _, _ = _kernel_case()
    n = A.shape[0]
    rng = np.random.default_rng(3)
    perm = rng.permutation(n).astype(np.int32)
    pos = np.argsort(perm)
    B = sp.csr_matrix((np.zeros(A.nnz), (pos[A.tocoo().row], pos[A.tocoo().col])), shape=A.shape)  # B[r, c] <- A[perm[r], perm[c]]
    B.sort_indices()
    sub = A.copy()
    sub.data[::3] = 0.0
    sub.eliminate_zeros()  # a proper sub-pattern
    for pat, rm, cm in ((A, None, None), (B, perm, perm), (sub, None, None)):
        want = ref.lookup_through_permutation(A, pat, rm, cm)
        assert None not in want
        assert rc.same_bits(mi.csr_reuse_op(1, A, pat, rowmap=rm, colmap=cm), np.array(want))
    # an entry the source does not store: the internal error from the status word, nothing written
    missing = A.tolil()
    r = 100
    c = next(j for j in range(n) if A[r, j] == 0)
    missing[r, c] = 1.0
    missing = missing.tocsr()
    missing.sort_indices()
    with pytest.raises(mi.HypreError) as e:
        mi.csr_reuse_op(1, A, missing)
    assert "internal error" in str(e.value) and e.value.bad_row == r and np.isnan(e.value.values).all()
    mi.call("HYPRE_ClearAllErrors")


def _child(mode, env=None, timeout=240):
    e = dict(os.environ, MI_HYPRE_DEVICE_SETUP_MIN_ROWS="64", **{k: str(v) for k, v in (env or {}).items()})
    p = subprocess.run([sys.executable, WORKER, mode], env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-4000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


@pytest.fixture(scope="module")
def plain_refresh():
    return _child("refresh", dict(MI_HYPRE_LOCALITY_ORDER=0))


def test_device_refresh_equals_host_only_refresh(plain_refresh):
    """the worker asserts the bits (A_l, Az, Ar, norms; cf, perm, P, R kept); here: several levels took the device path"""
    print(plain_refresh)
    assert min(plain_refresh["levels"]) >= 3 and min(plain_refresh["device_levels"]) >= 2
    assert plain_refresh["refreshed"] >= 2 * 2 * 5


def test_device_refresh_with_the_locality_numbering():
    r = _child("refresh", dict(MI_HYPRE_LOCALITY_ORDER=1))
    assert min(r["device_levels"]) >= 2


def test_poisoned_allocations_give_the_same_digest(plain_refresh):
    r = _child("refresh", dict(MI_HYPRE_LOCALITY_ORDER=0, MI_HYPRE_POISON_ALLOC=1))
    assert r["digest"] == plain_refresh["digest"]


@pytest.mark.parametrize("tail_rows", [None, 0])
def test_one_cycle_of_the_refreshed_hierarchy(tail_rows):
    """against the oracle's cycle on the reported refreshed levels at 1e-12 max|ref| (the tolerance of
    test_vcycle_matches_oracle).  Chebyshev, which the oracle does not have: the eigenvalue bounds of every refreshed
    level against the restatement of tests/cheby_ref.py, and the cycle against a fresh handle at the same tolerance
    after a refresh to 2 A (whose fresh interpolation is the kept one bit for bit).  With the coarse tail collapsed
    (default) and not.  2^k A gives exactly 2^-k times the default cycle."""
    r = _child("cycle", {} if tail_rows is None else dict(MI_HYPRE_DENSE_TAIL_ROWS=tail_rows))
    print(r)
    assert r["default"] <= 1e-12 and r["ilu"] <= 1e-12 and r["cheby"] <= 1e-12
    assert r["cheby_bounds_gap"] <= r["cheby_bounds_tol"]
    assert r["scaled_1"] and r["scaled_-3"]


def test_the_value_format_of_level_zero_follows_the_values():
    r = _child("dict")
    assert r["kinds"] == [8, 0, 8] and r["equal"] == [True, True]


def test_a_bound_krylov_solver_refreshes_and_converges():
    r = _child("krylov")
    print(r)
    for v in r.values():
        assert v["true_rel_res"] < 1e-8 and v["iters_fresh"] < 40 and v["iters_refreshed"] <= 100


def test_a_failed_refresh_leaves_the_handle_not_set_up():
    r = _child("failed")
    print(r)
    assert "zero pivot" in r["message"] and "returned 1:" in r["message"]
    assert r["kind_after_failure"] == [1, 1] and r["kind_then"] == [2, 0]
