"""GPU: the direct (level-scheduled) ILU(k) path -- symbolic pattern, ilu_factor_k, the exact and the Jacobi
substitutions, the Richardson solver on vectors and multivectors, re-setup, and the refusal of a missing or zero pivot
-- on the irregular matrices of tests/ilu_cases.py against the numpy reference of tests/ilu_ref.py (which
tests/test_ilu_spec.py checks on the CPU).  No oracle is called here.

Tolerance of every value comparison: max|device - longdouble| <= 4 * max|float64 restatement - longdouble| +
2 eps max|longdouble|.  The first term is the reference's own: what float64 in the device's operation order loses
against longdouble, measured on the CPU (the factor 4 allows for a division that rounds differently).  Measured
max|float64 - longdouble| (x86-64 longdouble, 64-bit mantissa), factors / exact application to the seeded vector:

    case      fill 0                fill 1                fill 2
    ragged    2.30e-14 / 1.72e-16   3.51e-14 / 3.39e-16   6.49e-14 / 6.14e-16    (max|factor| 2.5e+02)
    chain     3.29e-16 / 2.09e-16   3.78e-16 / 2.01e-16   3.78e-16 / 2.79e-16    (max|factor| 7.7e+00)
    arrow     5.27e-13 / 1.32e-16   2.78e-13 / 1.17e-16   4.67e-14 / 1.73e-16    (max|factor| 3.2e+02)
    onesided  1.19e-16 / 4.30e-16   5.59e-16 / 4.68e-16   9.26e-16 / 9.82e-16    (max|factor| 4.2e+00)
    wide      4.79e-16 / 3.30e-16
    tiny1-3   0 / <= 4.2e-17

Every input keeps its indices in range; no test relies on a fault."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import ilu_cases as ic
from tests import ilu_ref

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def _ij(mi, M):
    M = sp.csr_matrix(M)
    n = M.shape[0]
    A = mi.IJMatrix(0, n - 1)
    coo = M.tocoo()
    A.set_values_coo(coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data.astype(np.float64))
    A.assemble()
    return A


_MATS, _DEV = {}, {}


def _mat(mi, name):
    if name not in _MATS:
        _MATS[name] = _ij(mi, ic.matrix(name))
    return _MATS[name]


def _dev(mi, name, fill):
    """(IJ matrix, ILU set up once on it at this fill, its factors)"""
    if (name, fill) not in _DEV:
        A = _mat(mi, name)
        ilu = mi.ILU(max_iterations=1, tolerance=0.0, trisolve=1, fill=fill)
        ilu.setup(A)
        _DEV[(name, fill)] = (A, ilu) + tuple(ilu.factors())
    return _DEV[(name, fill)]


def _configure(mi, ilu, trisolve, its=(5, 5), max_iterations=1, tolerance=0.0):
    mi.call("HYPRE_ILUSetTriSolve", ilu.h, trisolve)
    mi.call("HYPRE_ILUSetLowerJacobiIters", ilu.h, int(its[0]))
    mi.call("HYPRE_ILUSetUpperJacobiIters", ilu.h, int(its[1]))
    mi.call("HYPRE_ILUSetMaxIter", ilu.h, max_iterations)
    mi.call("HYPRE_ILUSetTol", ilu.h, float(tolerance))


def _solve(mi, A, ilu, rhs):
    """HYPRE_ILUSolve on a zero guess; rhs of shape (n,) or (ncomp, n)"""
    rhs = np.asarray(rhs, dtype=np.float64)
    n = rhs.shape[-1]
    nc = 1 if rhs.ndim == 1 else rhs.shape[0]
    b = mi.IJVector(0, n - 1, rhs.copy(), ncomp=nc)
    x = mi.IJVector(0, n - 1, np.zeros_like(rhs), ncomp=nc)
    ilu.solve(A, b, x)
    return x.get() if nc == 1 else x.get_all()


def _apply(mi, name, fill, trisolve, its=(5, 5), rhs=None):
    A, ilu = _dev(mi, name, fill)[:2]
    _configure(mi, ilu, trisolve, its)
    return _solve(mi, A, ilu, ic.reference(name, fill).rhs if rhs is None else rhs)


def _held(got, f64, ld, what):
    dev, tol = ilu_ref.deviation(got, ld), ilu_ref.bound(f64, ld)
    print(f"{what}: max|device - longdouble| {dev:.3e}, bound {tol:.3e} (float64 restatement "
          f"{ilu_ref.deviation(f64, ld):.3e}), bit-equal to the restatement: {np.array_equal(got, f64)}")
    assert dev <= tol, (what, dev, tol)


@pytest.mark.parametrize("name,fill", ic.ALL, ids=ic.IDS)
def test_pattern_and_factors(mi, name, fill):
    R = ic.reference(name, fill)
    _, _, ia, ja, a = _dev(mi, name, fill)
    assert np.array_equal(ia, R.ia) and np.array_equal(ja, R.ja)
    _held(a, R.f64.a, R.ld.a, f"{name} fill {fill} factors")


@pytest.mark.parametrize("name,fill", ic.ALL, ids=ic.IDS)
def test_exact_substitutions(mi, name, fill):
    ld, f64 = ic.reference(name, fill).applied()
    _held(_apply(mi, name, fill, 1), f64, ld, f"{name} fill {fill} exact application")


@pytest.mark.parametrize("name,fill", ic.ALL, ids=ic.IDS)
def test_jacobi_substitutions(mi, name, fill):
    """Both parities of the buffer alternation at the end of IluSolver::apply, and the start kernels alone (0, 0)."""
    R = ic.reference(name, fill)
    for its in ic.JACOBI_ITS:
        ld, f64 = R.applied(its)
        _held(_apply(mi, name, fill, 0, its), f64, ld, f"{name} fill {fill} Jacobi {its}")


@pytest.mark.parametrize("name,fill", [(n, f) for n, f in ic.ALL if n in ("chain", "arrow")],
                         ids=[i for (n, f), i in zip(ic.ALL, ic.IDS) if n in ("chain", "arrow")])
def test_jacobi_at_the_nilpotency_bound_equals_the_exact_substitutions(mi, name, fill):
    R = ic.reference(name, fill)
    its = R.nilpotency_its()
    exact_ld = R.applied()[0]
    f64 = R.f64.apply_jacobi(R.rhs, *its)
    _held(_apply(mi, name, fill, 0, its), f64, exact_ld, f"{name} fill {fill} Jacobi {its} against the exact application")
    _held(_apply(mi, name, fill, 1), f64, exact_ld, f"{name} fill {fill} exact application, the same bound")


def _true_rel(A, x, b):
    """(||b - A x|| / ||b|| in longdouble, the rounding bound of a float64 evaluation of it): every residual entry
    is a sum of at most m + 1 terms, so its error is at most (m + 2) eps (|b| + |A| |x|)_i."""
    A = sp.csr_matrix(A)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    Ax = np.zeros(A.shape[0], dtype=ilu_ref.LD)
    np.add.at(Ax, rows, A.data.astype(ilu_ref.LD) * x.astype(ilu_ref.LD)[A.indices])
    r = b.astype(ilu_ref.LD) - Ax
    bn = np.sqrt(np.sum(b.astype(ilu_ref.LD) ** 2))
    m = int(np.diff(A.indptr).max())
    slack = (m + 2) * EPS * np.sqrt(np.sum((np.abs(b) + abs(A) @ np.abs(x)) ** 2)) / float(bn)
    return float(np.sqrt(np.sum(r * r)) / bn), float(slack)


def test_richardson_solve(mi):
    """ILU(0) as a solver on `ragged`: the iteration count of the float64 restatement (tests/test_ilu_spec.py shows it
    stops clear of the tolerance), and a solution held to the residual it reached."""
    M, R = ic.matrix("ragged"), ic.reference("ragged", 0)
    b = M @ np.ones(R.n)
    xr, it, rels = ilu_ref.richardson(M, R.f64, b, 200, 1e-8)
    A, ilu = _dev(mi, "ragged", 0)[:2]
    _configure(mi, ilu, 1, max_iterations=200, tolerance=1e-8)
    x = _solve(mi, A, ilu, b)
    rel, slack = _true_rel(M, x, b)
    print(f"Richardson: {ilu.num_iterations} iterations (reference {it}), reported {ilu.final_rel_res:.6e}, "
          f"reference {rels[-1]:.6e}, true {rel:.6e} +- {slack:.1e}")
    assert ilu.num_iterations == it
    assert rel <= 1e-8 and abs(ilu.final_rel_res - rel) <= slack
    assert abs(rels[-1] - _true_rel(M, xr[0], b)[0]) <= slack


def test_multivector(mi):
    """ncomp = 3 on `ragged`: one application is three single-component applications, bit for bit; a solve to a
    tolerance stops on the one norm over all components (alone, the components need 5, 1 and 5 steps)."""
    M, R = ic.matrix("ragged"), ic.reference("ragged", 0)
    B = ic.multivector_rhs()
    A, ilu = _dev(mi, "ragged", 0)[:2]
    for tri, its in ((1, (5, 5)), (0, (2, 3))):
        _configure(mi, ilu, tri, its)
        together = _solve(mi, A, ilu, B)
        for c in range(3):
            assert np.array_equal(together[c], _solve(mi, A, ilu, B[c])), (tri, c)
    ld = np.stack([R.ld.apply_exact(B[c]) for c in range(3)])
    f64 = np.stack([R.f64.apply_exact(B[c]) for c in range(3)])
    _configure(mi, ilu, 1)
    _held(_solve(mi, A, ilu, B).ravel(), f64.ravel(), ld.ravel(), "ragged fill 0 multivector application")
    xr, it, rels = ilu_ref.richardson(M, R.f64, B, 200, 1e-8, ncomp=3)
    _configure(mi, ilu, 1, max_iterations=200, tolerance=1e-8)
    x = _solve(mi, A, ilu, B)
    K = sp.kron(sp.identity(3), M).tocsr()
    rel, slack = _true_rel(K, x.ravel(), B.ravel())
    print(f"multivector Richardson: {ilu.num_iterations} iterations (reference {it}), reported "
          f"{ilu.final_rel_res:.6e}, reference {rels[-1]:.6e}, true {rel:.6e} +- {slack:.1e}")
    assert ilu.num_iterations == it
    assert rel <= 1e-8 and abs(ilu.final_rel_res - rel) <= slack
    # a second solve with the kept residual buffer gives the same bits
    assert np.array_equal(_solve(mi, A, ilu, B), x)


def test_a_second_setup_on_another_matrix_is_a_fresh_setup(mi):
    """One ILU object: ILU(1) with Jacobi solves on `ragged`, then ILU(2) with exact solves on `chain` (another n,
    fill and trisolve), with a multivector solve to a tolerance on each (the kept residual buffer changes size)."""
    first, second = ic.reference("ragged", 1), ic.reference("chain", 2)
    B1 = ic.multivector_rhs()
    B2 = np.stack([second.rhs, 2.0 * second.rhs[::-1], ic.matrix("chain") @ np.ones(second.n)])

    def run(ilu, A, R, tri, its, B):
        out = list(ilu.factors())
        _configure(mi, ilu, tri, its)
        out.append(_solve(mi, A, ilu, R.rhs))
        _configure(mi, ilu, tri, its, max_iterations=200, tolerance=1e-8)
        out.append(_solve(mi, A, ilu, B))
        out.append(ilu.num_iterations)
        return out

    A1, A2 = _mat(mi, "ragged"), _mat(mi, "chain")
    reused = mi.ILU(fill=1, trisolve=0)
    reused.setup(A1)
    got1 = run(reused, A1, first, 0, (2, 3), B1)
    mi.call("HYPRE_ILUSetLevelOfFill", reused.h, 2)
    reused.setup(A2)
    got2 = run(reused, A2, second, 1, (5, 5), B2)
    for got, (A, R, fill, tri, its, B) in ((got1, (A1, first, 1, 0, (2, 3), B1)), (got2, (A2, second, 2, 1, (5, 5), B2))):
        fresh = mi.ILU(fill=fill, trisolve=tri)
        fresh.setup(A)
        want = run(fresh, A, R, tri, its, B)
        assert got[5] == want[5] and 0 < got[5] < 200
        for g, w in zip(got[:5], want[:5]):
            assert np.array_equal(g, w)
        fresh.destroy()
    assert np.array_equal(got2[0], second.ia) and np.array_equal(got2[1], second.ja)
    _held(got2[2], second.f64.a, second.ld.a, "chain fill 2 factors after a setup on ragged")
    _held(got2[3], second.applied()[1], second.applied()[0], "chain fill 2 application after a setup on ragged")
    reused.destroy()


@pytest.mark.parametrize("kind", ["missing", "stored_zero", "eliminated"])
def test_setup_refuses_a_missing_or_zero_pivot(mi, kind):
    """HYPRE_ILUSetup ends with an error that names the local row, at fills 0 and 1 and for both kinds of solve; the
    object is not set up afterwards, and the same object sets up on a good matrix."""
    M, bad = ic.refused(kind)
    good = ic.refused("good")[0]
    A, G = _ij(mi, M), _ij(mi, good)
    for fill in (0, 1):
        for tri in (0, 1):
            ilu = mi.ILU(fill=fill, trisolve=tri)
            with pytest.raises(mi.HypreError, match=rf"zero pivot u_jj in row {bad} of this rank's block \(global row {bad}\)"):
                ilu.setup(A)
            mi.call("HYPRE_ClearAllErrors")
            with pytest.raises(mi.HypreError, match="not set up"):
                ilu.factors()
            mi.call("HYPRE_ClearAllErrors")
            ilu.setup(G)
            _configure(mi, ilu, tri)
            # the blocks of the good matrix are at most 2x2: ILU(0) is its LU, one Jacobi sweep is exact
            assert np.abs(_solve(mi, G, ilu, good @ np.ones(6)) - 1.0).max() <= 8 * EPS
            ilu.destroy()


@pytest.mark.parametrize("kind", ["missing", "stored_zero", "eliminated"])
def test_boomeramg_setup_refuses_an_ilu_smoother_without_a_pivot(mi, kind):
    """The same 6x6 blocks in front of a 7-point Laplacian (so that the hierarchy has a level with a smoother):
    HYPRE_BoomerAMGSetup fails in the ILU smoother's setup; after HYPRE_ClearAllErrors the same object sets up and
    solves on the good matrix."""
    from tests import itilu_ref

    Lp = itilu_ref.laplace(8, 7)
    n = 6 + Lp.shape[0]
    bad_A = _ij(mi, sp.block_diag((ic.refused(kind)[0], Lp), format="csr"))
    good = sp.block_diag((ic.refused("good")[0], Lp), format="csr")
    good_A = _ij(mi, good)
    for fill in (0, 1):
        for tri in (0, 1):
            amg = mi.BoomerAMG(print_level=0, smooth_type=5, smooth_num_levels=1, ilu_level=fill, ilu_tri_solve=tri)
            with pytest.raises(mi.HypreError, match="HYPRE_BoomerAMGSetup.*zero pivot u_jj in row"):
                amg.setup(bad_A)
            mi.call("HYPRE_ClearAllErrors")
            amg.setup(good_A)
            assert amg.num_levels >= 2
            b = mi.IJVector(0, n - 1, good @ np.ones(n))
            x = mi.IJVector(0, n - 1, np.zeros(n))
            gm = mi.GMRES(tolerance=1e-9, max_iterations=100, kspace=50, print_level=0)
            gm.set_precond(amg)
            gm.setup(good_A, b, x)
            gm.solve(good_A, b, x)
            assert gm.final_rel_res < 1e-9 and np.abs(x.get() - 1.0).max() < 1e-6
            gm.destroy()
            amg.destroy()
