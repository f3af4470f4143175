"""CPU: the numpy restatement of the iterative ILU(0) setup (tests/itilu_ref.py) -- start value,
synchronous sweeps and norms -- and its convergence to the exact ILU(0) factors."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import itilu_ref


def _cases():
    return {"7pt": itilu_ref.laplace(6, 7), "27pt": itilu_ref.laplace(5, 27), "nonsym": itilu_ref.nonsymmetric(300)}


def test_start_value():
    A = sp.csr_matrix(np.array([[4.0, 1.0, 0.0], [2.0, 5.0, 1.0], [0.0, 3.0, 8.0]]))
    P = itilu_ref.Plan(A)
    x = P.start()
    # L: a_ij / a_jj below the diagonal, U: A's upper part
    assert np.array_equal(P.csr(x).toarray(), np.array([[4.0, 1.0, 0.0], [0.5, 5.0, 1.0], [0.0, 0.6, 8.0]]))


def test_pairs_of_a_small_pattern():
    A = sp.csr_matrix(np.array([[4.0, 1.0, 1.0], [2.0, 5.0, 1.0], [1.0, 3.0, 8.0]]))
    P = itilu_ref.Plan(A)
    # (2,2) sums l_20 u_02 and l_21 u_12; (1,0) and (0,*) sum nothing
    e22 = 8
    assert P.npairs[e22] == 2
    assert list(P.pl[e22, :2]) == [6, 7] and list(P.pu[e22, :2]) == [2, 5]
    assert P.npairs[3] == 0 and P.npairs[0] == 0


def test_one_sweep_by_hand():
    A = sp.csr_matrix(np.array([[4.0, 1.0], [2.0, 5.0]]))
    P = itilu_ref.Plan(A)
    x1 = P.sweep(P.start())
    # l_10 = a_10 / u_00 = 0.5, u_11 = a_11 - l_10(x_0) u_01(x_0) = 5 - 0.5 * 1
    assert np.array_equal(x1, np.array([4.0, 1.0, 0.5, 4.5]))
    assert P.correction(P.start(), x1) == pytest.approx(0.5 / 4.5)


@pytest.mark.parametrize("name", ["7pt", "27pt", "nonsym"])
def test_sweeps_converge_to_the_exact_factors(name):
    A = _cases()[name]
    P = itilu_ref.Plan(A)
    exact = itilu_ref.exact_ilu0(A)
    x = P.start()
    c = []
    for _ in range(60):
        xn = P.sweep(x)
        c.append(P.correction(x, xn))
        x = xn
    assert np.abs(x - exact).max() <= 1e-12 * np.abs(exact).max()
    assert c[-1] <= 1e-12 and P.residual(x) <= 1e-13
    # the exact factors are a fixed point of the sweep, bit for bit
    assert np.array_equal(P.sweep(exact), exact)


def test_exact_ilu0_reproduces_a_on_its_pattern():
    A = itilu_ref.nonsymmetric(200, seed=3)
    P = itilu_ref.Plan(A)
    v = itilu_ref.exact_ilu0(A)
    F = P.csr(v)
    L = sp.tril(F, -1) + sp.identity(A.shape[0])
    U = sp.triu(F)
    LU = (L @ U).tocsr()
    d = np.abs(np.asarray(LU[P.row, P.col]).ravel() - P.a).max()
    assert d <= 1e-13 * np.abs(P.a).max()


def test_stop_sweep_matches_the_correction_sequence():
    A = itilu_ref.laplace(6, 27)
    P = itilu_ref.Plan(A)
    m = P.stop_sweep(1e-6, 50)
    x = P.run(m - 1)
    assert P.correction(x, P.sweep(x)) <= 1e-6
    if m > 1:
        y = P.run(m - 2)
        assert P.correction(y, P.sweep(y)) > 1e-6
