"""CPU: the numpy ILU(k) reference of tests/ilu_ref.py held to properties that do not depend on it, and the oracle held
to the reference, on the irregular cases of tests/ilu_cases.py.  tests/test_gpu_ilu_irregular.py compares the device with
this reference; here is what that comparison rests on."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import ilu_cases as ic
from tests import ilu_ref

EPS = np.finfo(np.float64).eps
SMALL = [(name, fill) for name, fill in ic.ALL if name != "wide"]
SMALL_IDS = [f"{name}-fill{fill}" for name, fill in SMALL]


def _dense_pattern(R):
    pat = np.zeros((R.n, R.n), dtype=bool)
    pat[np.repeat(np.arange(R.n), np.diff(R.ia)), R.ja] = True
    return pat


def test_the_cases_are_what_they_are_named_for():
    A = ic.matrix("ragged")
    ln = np.diff(A.indptr)
    off = np.asarray(abs(A).sum(axis=1)).ravel() - np.abs(A.diagonal())
    assert A.shape == (600, 600) and (np.abs(A.diagonal()) > off).all() and (A != A.T).nnz > 0
    assert (ln == 1).sum() >= 4 and ln.max() >= 290 and np.diff(A.tocsc().indptr).max() >= 290
    assert set(range(1, 31)) <= set(ln.tolist()) and np.sort(ln)[-2] <= 31
    assert (A.data > 0).any() and (A.data < 0).any() and (A.diagonal() > 0).any() and (A.diagonal() < 0).any()
    A = ic.matrix("chain")
    assert (A.diagonal(-1) != 0).all() and sp.tril(A, -2).nnz == 0
    for fill in (0, 1, 2):
        assert ic.reference("chain", fill).levels[0] == 300  # one row per lower level set
    R = ic.reference("wide", 0)
    assert R.n == 2053 and R.levels == (3, 3)
    first = sum(1 for i in range(R.n) if not (R.ja[R.ia[i]:R.ia[i + 1]] < i).any())
    assert first > 256 and first % 256 != 0  # several workgroups, the last partly filled
    A = ic.matrix("arrow")
    assert np.diff(A.indptr)[-1] == 400 and np.diff(A.tocsc().indptr)[-1] == 400
    A = ic.matrix("onesided")
    off = A - sp.diags(A.diagonal())
    assert off.multiply(off.T).nnz == 0  # a_ij stored only where a_ji is not
    assert (np.abs(A.diagonal()) < np.asarray(abs(off).sum(axis=1)).ravel()).sum() > 400  # not diagonally dominant
    assert sp.tril(ic.matrix("tiny3"), -1).nnz == 0 and ic.matrix("tiny2").nnz == 4 and ic.matrix("tiny1").shape == (1, 1)


@pytest.mark.parametrize("fill", [0, 1, 2])
def test_onesided_stays_away_from_pivot_breakdown(fill):
    R = ic.reference("onesided", fill)
    piv = np.abs(R.ld.a[R.ld.dpos]).min()
    assert piv >= 1e-3 * np.abs(R.A.data).max(), float(piv)


@pytest.mark.parametrize("name", sorted(ic.BUILDERS))
def test_ilu0_reproduces_a_on_its_pattern(name):
    """(L U)_ij == a_ij on the pattern of A; on the fill of ILU(k) the product is 0 (a_ij = 0 there)."""
    for fill in ic.FILLS[name]:
        R = ic.reference(name, fill)
        row = np.repeat(np.arange(R.n), np.diff(R.ia))
        F = sp.csr_matrix((R.ld.a.astype(np.float64), R.ja, R.ia), shape=(R.n, R.n))
        L = (sp.tril(F, -1) + sp.identity(R.n)).tocsr()
        U = sp.triu(F).tocsr()
        P = (L @ U).tocsr()
        got = np.asarray(P[row, R.ja]).ravel()
        want = np.asarray(R.A.tocsr()[row, R.ja]).ravel()
        # a few ulp of the largest term of an entry's sum
        scale = np.asarray((abs(L) @ abs(U)).tocsr()[row, R.ja]).ravel()
        assert (np.abs(got - want) <= 8 * EPS * np.maximum(scale, np.abs(want))).all(), (name, fill)


@pytest.mark.parametrize("name", ["onesided", "bordered", "chain", "tiny2", "tiny3"])
def test_full_fill_is_the_dense_lu_without_pivoting(name):
    """With fill >= n nothing is dropped: L and U are the dense LU without pivoting, zero outside the pattern.  Where
    the first row and column are full ('bordered', tiny2) every entry fills and the pattern is the full square."""
    A = ic.matrix("onesided" if name == "bordered" else name)
    if A.shape[0] > 120:  # the leading block: the same structure, and a dense Doolittle loop stays quick
        A = A[:120, :120].tolil()
        if name == "bordered":
            A[0, 1:] = 0.25
            A[1:, 0] = -0.25
        A = A.tocsr()
    n = A.shape[0]
    ia, ja = ilu_ref.symbolic(A, n)
    if name in ("bordered", "tiny2"):
        assert len(ja) == n * n
    F = ilu_ref.Factors(A, n, ilu_ref.LD, pattern=(ia, ja))
    L, U = F.dense_LU()
    D = A.toarray().astype(ilu_ref.LD)
    Ld, Ud = np.eye(n, dtype=ilu_ref.LD), np.zeros((n, n), dtype=ilu_ref.LD)
    for i in range(n):  # Doolittle: row i of U, then column i of L, as inner products
        Ud[i, i:] = D[i, i:] - Ld[i, :i] @ Ud[:i, i:]
        Ld[i + 1:, i] = (D[i + 1:, i] - Ld[i + 1:, :i] @ Ud[:i, i]) / Ud[i, i]
    tol = 64 * n * np.finfo(ilu_ref.LD).eps * max(float(np.abs(Ld).max()), 1.0) * float(np.abs(Ud).max())
    assert float(np.abs(L - Ld).max()) <= tol and float(np.abs(U - Ud).max()) <= tol
    assert float(np.abs(L @ U - D).max()) <= tol


@pytest.mark.parametrize("name", ["ragged", "chain", "arrow", "onesided"])
def test_the_patterns_nest_as_fill_grows(name):
    pats = [_dense_pattern(ic.reference(name, fill)) for fill in (0, 1, 2)]
    A = ic.matrix(name).tocoo()
    base = np.zeros_like(pats[0])
    base[A.row, A.col] = True
    assert np.array_equal(pats[0], base)
    assert not (pats[0] & ~pats[1]).any() and not (pats[1] & ~pats[2]).any()
    assert pats[1].sum() > pats[0].sum() and pats[2].sum() > pats[1].sum()


NILPOTENT = [(name, fill) for name, fill in SMALL if name != "ragged" or fill == 0]  # (ragged with fill: seconds)


@pytest.mark.parametrize("name,fill", NILPOTENT, ids=[f"{name}-fill{fill}" for name, fill in NILPOTENT])
def test_jacobi_at_the_nilpotency_bound_is_the_exact_application(name, fill):
    """The strict triangles are nilpotent: after (level sets - 1) sweeps the Jacobi form has the substitution's value,
    up to rounding.  A single lower sweep on the chain does not."""
    R = ic.reference(name, fill)
    F = R.ld
    exact = R.applied()[0]
    its = R.nilpotency_its()
    z = F.apply_jacobi(R.rhs, *its)
    top = float(np.abs(exact).max())
    assert float(np.abs(z - exact).max()) <= 1e3 * R.n * float(np.finfo(ilu_ref.LD).eps) * top, (name, fill)
    if name == "chain":
        short = F.apply_jacobi(R.rhs, 1, its[1])
        assert float(np.abs(short - exact).max()) > 1e-6 * top


@pytest.mark.parametrize("name,fill", ic.ALL, ids=ic.IDS)
def test_the_oracle_agrees_with_the_reference(oc, name, fill):
    """Pattern equality, and values within the float64 restatement's own distance from the longdouble reference (the
    bound of the GPU tests): the oracle is not wrong in the way the library could be."""
    R = ic.reference(name, fill)
    for tri, its in ((1, None), (0, (2, 3)), (0, (0, 0))):
        lit, uit = its or (5, 5)
        ilu = oc.Ilu(oc.Csr.from_scipy(R.A), tri_solve=tri, lower_it=lit, upper_it=uit, level_of_fill=fill)
        F = ilu.factor().to_scipy()
        assert np.array_equal(F.indptr, R.ia) and np.array_equal(F.indices, R.ja)
        assert ilu_ref.deviation(F.data, R.ld.a) <= ilu_ref.bound(R.f64.a, R.ld.a)
        ld, f64 = R.applied(its)
        assert ilu_ref.deviation(ilu.apply(R.rhs), ld) <= ilu_ref.bound(f64, ld), (tri, its)


def test_the_richardson_reference_stops_clear_of_the_tolerance():
    """The iteration counts the GPU tests compare are not a matter of rounding: the test that stops the loop passes by
    more than 1 %, and the one before fails by more; the multivector stops later than its quickest component would alone."""
    A, R = ic.matrix("ragged"), ic.reference("ragged", 0)
    b = A @ np.ones(R.n)
    x, it, rels = ilu_ref.richardson(A, R.f64, b, 200, 1e-8)
    assert 3 <= it < 200 and rels[-1] <= 0.99e-8 and rels[-2] >= 1.01e-8
    assert np.abs(x - 1.0).max() <= 1e-6
    B = ic.multivector_rhs()
    xm, itm, relm = ilu_ref.richardson(A, R.f64, B, 200, 1e-8, ncomp=3)
    assert relm[-1] <= 0.99e-8 and relm[-2] >= 1.01e-8
    each = [ilu_ref.richardson(A, R.f64, B[c], 200, 1e-8)[1] for c in range(3)]
    assert min(each) < itm < 200 and len(set(each)) > 1, (each, itm)
