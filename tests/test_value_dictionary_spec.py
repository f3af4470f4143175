"""CPU: what tests/dict_cases.py claims about its operators, and the reference of tests/test_gpu_value_dictionary.py.

The GPU tests can only pin the value-dictionary kernels if their operators really get a dictionary (x cache: mean row
length >= 3; 65536 entries; at most 256 distinct bit patterns), really take the launch geometry they are named after
(tile Gauss-Seidel: mean > 5; 512 threads: mean >= 100; lanes per row by the tile's row count; more than 1024 unique
columns in a tile; a row longer than its tile) and, for the refusals, really hide the deciding value from the sample."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import dict_cases as dc


@pytest.fixture(scope="module")
def relax_ops():
    return {name: dc.relax_case(name) for name in list(dc.RELAX) + [z for z in dc.ZERO if z not in dc.RELAX]}


def _mean(M):
    return M.nnz / M.shape[0]


@pytest.mark.parametrize("name", list(dc.RELAX) + ["rowlen17-12003", "ragged-16001"])
def test_relaxation_operators(oc, relax_ops, name):
    M = relax_ops[name]
    kind, n, nd = dc.RELAX.get(name) or dc.ZERO[name]
    assert M.shape == (n, n) and n % 8 != 0 and M.has_sorted_indices
    assert dc.distinct(M) == nd == len(np.unique(dc.bits(M.data)))
    assert M.nnz >= dc.THRESHOLD
    if name in ("rowlen7", "rowlen17", "rowlen33", "ragged", "wide"):  # the smallest size: 2 % more rows at the most
        assert M.nnz < 1.02 * dc.THRESHOLD
    # M-matrix, symmetric, dominant diagonal that is a power of two and takes few values
    d = M.diagonal()
    off = (M - sp.diags(d)).tocsr()
    off.eliminate_zeros()
    assert (off.data < 0).all() and (d > 0).all() and abs(M - M.T).nnz == 0
    rowsum = np.abs(off).sum(axis=1).A1
    assert np.all(d >= 1.01 * rowsum) and np.all(d < 2.03 * np.maximum(rowsum, 0.5))
    assert np.array_equal(np.log2(d), np.round(np.log2(d))) and len(np.unique(d)) <= 6
    # both halves of the table, and values that are no floats
    assert (M.data < 0).any() and (M.data > 0).any()
    vals = np.unique(M.data)
    assert (vals.astype(np.float32).astype(np.float64) != vals).sum() >= 0.9 * (len(vals) - 6)
    # thresholds: x cache, tile Gauss-Seidel, wide tiles
    L = np.diff(M.indptr)
    assert _mean(M) > 5.0 and (_mean(M) >= 100.0) == (kind == "wide")
    if kind == "ragged":
        assert L.min() == 1 and L.max() <= 13 and np.all(L[::17] == 1)
    elif kind == "wide":
        assert 101 <= L.min() and L.max() <= 301
    elif kind == "scattered":
        assert 7.0 < _mean(M) - 1.0 < 9.0 and n >= 20000
    else:
        s = dc.STRIDES[kind]
        assert L.max() == 2 * s + 2 and (L >= 2 * s + 1).sum() >= (1000 if s >= 32 else 400)  # (+ 1: a planted coupling)
    # the hierarchy the relaxation tests compare with, and the geometry of level 0 in ITS ordering
    o = oc.Amg(oc.Csr.from_scipy(M), oc.default_params(gs_chunk=8))
    assert o.num_levels > 1
    A0 = o.level_A(0).to_scipy().tocsr()
    A0.sort_indices()
    cf = o.level_cf(0)
    nc = int((cf == 1).sum())
    assert 0 < nc < n and np.all(cf[:nc] == 1) and np.all(cf[nc:] == -1)
    assert np.array_equal(np.sort(dc.bits(A0.data)), np.sort(dc.bits(M.data)))
    t = dc.tile_census(A0)
    assert t["block"] == (512 if kind == "wide" else 256) and t["entries"].max() < t["tile"] and len(t["rows"]) > 1
    coo = A0.tocoo()
    coupled = np.unique(coo.row[(coo.row // 8 == coo.col // 8) & (coo.row != coo.col)] // 8)
    nchunks = (n + 7) // 8
    print(f"{name}: nnz {M.nnz}, mean {_mean(M):.1f}, nc {nc}, tiles {len(t['rows'])}, lanes per row "
          f"{dict(zip(*np.unique(t['lpr'], return_counts=True)))}, coupled chunks {len(coupled)} of {nchunks}, "
          f"most unique columns {t['unique'].max()}")
    assert 0 < len(coupled) < nchunks  # chunks on the general sweep and chunks on the diagonal path
    if kind in dc.LPR:
        assert (t["lpr"] == dc.LPR[kind]).sum() >= 10
        assert len(coupled) < nchunks // 4  # the strides keep most chunks diagonal
    if kind == "wide":
        assert np.all(t["lpr"] == 8)
    if kind == "scattered":
        assert (t["unique"] > 1024).sum() >= 0.9 * len(t["unique"])
    # the zero-guess sub-operator: the entries inside the rows' chunks, and the C columns of the F rows
    az = int(((coo.row // 8 == coo.col // 8) | ((coo.row >= nc) & (coo.col < nc))).sum())
    if name == "ragged-16001":
        assert az >= dc.THRESHOLD and az / n >= 3.0
    if kind in dc.STRIDES:
        assert az / n < 3.0  # no x cache: this sub-operator never has a dictionary


@pytest.mark.parametrize("name", list(dc.SPMV) + list(dc.GIANT))
def test_spmv_operators(name):
    M, info = dc.spmv_case(name)
    kind, n, nd = (dc.SPMV.get(name) or dc.GIANT[name])[:3]
    L = np.diff(M.indptr)
    assert M.has_sorted_indices and n % 8 != 0 and dc.distinct(M) == nd and info["kind"] == 8
    assert M.nnz >= dc.THRESHOLD and _mean(M) >= 3.0 and (_mean(M) >= 100.0) == (kind == "wide")
    assert (M.data < 0).any() and (M.data > 0).any()
    vals = np.unique(M.data)
    assert (vals.astype(np.float32).astype(np.float64) != vals).sum() >= 0.75 * len(vals)
    t = dc.tile_census(M)
    if kind == "ragged":
        assert (L == 0).sum() >= n // 17 and np.all(L[::17][: n // 17] == 0)  # truly empty rows
        assert len(np.unique(M.indptr[t["rb"][:-1]] % 2)) == 2  # tiles that start on odd and on even stored positions
    if name == "scattered":
        assert (t["unique"] > 1024).sum() >= 0.9 * len(t["unique"])
    if name == "rowlen33":
        assert (t["unique"] > 1024).sum() >= 0.9 * len(t["unique"])
    if name in dc.GIANT:
        r = n // 2 + 3
        assert L[r] == info["giant"] > t["tile"] and L[r] == L.max() and np.sort(L)[-2] < t["tile"] // 8
        k = int(np.searchsorted(t["rb"], r))
        assert t["rb"][k] == r and t["rb"][k + 1] == r + 1  # a tile of its own
    else:
        assert t["entries"].max() < t["tile"]


@pytest.mark.parametrize("name", dc.REFUSALS)
def test_refusal_operators(name):
    M, info = dc.spmv_case(name)
    nnz, n = M.nnz, M.shape[0]
    assert M.has_sorted_indices and _mean(M) >= 3.0 and _mean(M) < 100.0
    pos = dc.sample_positions(nnz)
    assert len(pos) == min(nnz, dc.THRESHOLD) and pos[-1] < nnz
    seen = np.unique(dc.bits(M.data[pos])) if nnz >= dc.THRESHOLD else None
    if name == "distinct257":
        assert dc.THRESHOLD < nnz < 2 * dc.THRESHOLD and len(seen) == 257 == dc.distinct(M) and info["kind"] == 0
    elif name == "distinct256":
        assert dc.THRESHOLD < nnz < 2 * dc.THRESHOLD and len(seen) == 256 == dc.distinct(M) and info["kind"] == 8
        table = np.sort(dc.bits(np.unique(M.data)))
        at = np.flatnonzero(dc.bits(M.data) == table[255])
        assert table[255] == dc.bits(np.array([info["top"]]))[0] and (at % 2 == 0).any() and (at % 2 == 1).any()
    elif name in ("tail_miss", "stride_miss"):
        at = np.flatnonzero(M.data == info["extra"])
        assert len(at) >= 2 and not np.isin(at, pos).any() and info["kind"] == 0
        assert len(seen) == 20 and dc.distinct(M) == 21
        if name == "tail_miss":
            assert dc.THRESHOLD < nnz < 2 * dc.THRESHOLD and nnz // dc.THRESHOLD == 1 and at.min() == dc.THRESHOLD
        else:
            assert 2 * dc.THRESHOLD <= nnz < 3 * dc.THRESHOLD and nnz // dc.THRESHOLD == 2 and np.all(at % 2 == 1)
            assert at.min() < dc.THRESHOLD  # hidden by the stride, not by lying behind the sample
    else:
        other, _ = dc.spmv_case("below_threshold" if name == "at_threshold" else "at_threshold")
        assert nnz == (dc.THRESHOLD if name == "at_threshold" else dc.THRESHOLD - 1)
        assert info["kind"] == (8 if name == "at_threshold" else 0) and dc.distinct(M) <= 40
        k = min(nnz, other.nnz)  # the same operator but for the last entry
        assert other.shape == M.shape and np.array_equal(M.data[:k], other.data[:k])
        assert np.array_equal(M.indices[:k], other.indices[:k]) and abs(nnz - other.nnz) == 1


@pytest.mark.parametrize("name", list(dc.PENDANT))
def test_pendant_operator_has_the_coarse_level_it_promises(oc, name):
    """level 1 of the oracle's hierarchy is A1 bit for bit: a dictionary operator (65536 entries, at most 256 values, most
    of them no floats, a diagonal that IS made of floats) on a level that fp32 value storage narrows"""
    M, A1 = dc.pendant_operator(name)
    ns = A1.shape[0]
    assert M.shape[0] == 3 * ns and abs(M - M.T).nnz == 0 and dc.distinct(M) <= 256 and M.nnz >= dc.THRESHOLD
    o = oc.Amg(oc.Csr.from_scipy(M), oc.default_params(gs_chunk=8))
    assert o.num_levels > 2
    nc = int((o.level_cf(0) == 1).sum())
    assert nc == ns and np.array_equal(o.level_perm(0)[:nc], np.arange(ns))  # the C points: S's rows, in order
    L1, p1 = o.level_A(1).to_scipy().tocsr(), o.level_perm(1)
    inv = np.empty_like(p1)
    inv[p1] = np.arange(ns)
    U = L1[inv][:, inv].tocsr()
    U.sort_indices()
    assert np.array_equal(U.indptr, A1.indptr) and np.array_equal(U.indices, A1.indices)
    assert np.array_equal(dc.bits(U.data), dc.bits(A1.data))
    assert A1.nnz >= dc.THRESHOLD and 2 < dc.distinct(A1) <= 256 and _mean(A1) > 5.0
    assert (_mean(A1) >= 100.0) == (name == "wide")
    d = A1.diagonal()
    off = (A1 - sp.diags(d)).tocsr()
    off.eliminate_zeros()
    assert (off.data < 0).all() and np.all(d > np.abs(off).sum(axis=1).A1)
    R = dc.rounded(A1)
    assert np.array_equal(R.diagonal(), d) and (R.data != A1.data).sum() >= 0.9 * off.nnz
    for X in (A1, R):  # the oracle hierarchy of the level alone: the same splitting, so its level 0 stands for level 1
        o1 = oc.Amg(oc.Csr.from_scipy(X), oc.default_params(gs_chunk=8))
        assert o1.num_levels > 1
        assert np.array_equal(o1.level_cf(0), o.level_cf(1)) and np.array_equal(o1.level_perm(0), p1)


def test_reference_against_a_dense_long_double_product():
    """200 rows: reference_matvec against the dense float128 product, and its bound against the same product in fp64 in
    three summation orders"""
    M = dc.palette_operator("ragged", 201, 50, 3, mmatrix=False, empty_rows=True)[:200, :200].tocsr()
    rng = np.random.default_rng(4)
    x, b = rng.standard_normal(200), rng.standard_normal(200)
    D = M.toarray().astype(np.float128)
    for alpha, beta in ((1.0, 0.0), (-1.5, 0.75)):
        ref, bound = dc.reference_matvec(M, x, alpha, beta, b)
        dense = np.float128(alpha) * (D @ x.astype(np.float128)) + np.float128(beta) * b.astype(np.float128)
        scale = abs(alpha) * (np.abs(D) @ np.abs(x).astype(np.float128)) + np.abs(np.float128(beta) * b)
        assert ref.dtype == np.float128 and np.all(np.abs(ref - dense) <= 2.0 ** -60 * scale)
        L = np.diff(M.indptr)
        want = (L + 3) * np.float128(2.0) ** -53 * scale
        assert np.all(np.abs(bound - want) <= 2.0 ** -50 * want) and np.all(bound[L > 0] > 0)
        Md = M.toarray()
        for y in (alpha * (M @ x) + beta * b, alpha * (Md @ x) + beta * b, alpha * (Md[:, ::-1] @ x[::-1]) + beta * b):
            assert np.all(np.abs(y - ref) <= bound)
        wrong = alpha * (M @ x) + beta * b
        wrong[7] += 64 * float(bound[7]) + 1e-300
        assert not np.all(np.abs(wrong - ref) <= bound)
