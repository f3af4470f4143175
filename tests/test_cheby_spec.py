"""CPU: the restatement of the Chebyshev relaxation (tests/cheby_ref.py) against itself and
scipy, and the parts of relax type 16 that need no device: the kernel choice, the exported symbols, the host-only
refusal."""
import ctypes

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp

from tests import cheby_ref


def _spd(n, seed, density=0.2):
    rng = np.random.default_rng(seed)
    M = sp.random(n, n, density=density, random_state=rng, format="csr")
    M = (M + M.T).tocsr()
    M.setdiag(0.0)
    M.eliminate_zeros()
    M = M - sp.diags(M.diagonal())
    # off-diagonals of both signs, strictly diagonally dominant with an uneven diagonal
    M.data = M.data - 0.5
    return (M + sp.diags(abs(M).sum(axis=1).A1 * (1.05 + rng.random(n)) + 0.1)).tocsr()


def laplace(n, stencil=7):
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n))
    I = sp.identity(n)
    if stencil == 7:
        return (sp.kron(sp.kron(I, I), T) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(T, I), I)).tocsr()
    S = sp.diags([1.0, 1.0, 1.0], [-1, 0, 1], shape=(n, n))
    return (27.0 * sp.identity(n ** 3) - sp.kron(sp.kron(S, S), S)).tocsr()


@pytest.mark.parametrize("order", [1, 2, 3, 4])
@pytest.mark.parametrize("eig_est", [0, 10])
def test_recurrence_equals_closed_form(order, eig_est):
    A = _spd(40, 3)
    bd = cheby_ref.level_bounds(A, eig_est)
    rng = np.random.default_rng(order)
    f, u = rng.standard_normal(40), rng.standard_normal(40)
    for guess in (u, None):
        got = cheby_ref.sweep(A, f, guess, bd["theta"], bd["delta"], order)
        ref = cheby_ref.sweep_closed_form(A, f, guess, bd["theta"], bd["delta"], order)
        # the recurrence in float64 against the polynomial in longdouble: a few roundings per step
        assert np.abs(got - ref.astype(np.float64)).max() <= 1e-13 * np.abs(ref).max()


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_residual_polynomial_is_bounded_on_the_interval(order):
    theta, delta = 1.3, 0.7
    q = cheby_ref.residual_polynomial(theta, delta, order)
    lam = np.linspace(theta - delta, theta + delta, 2001).astype(np.longdouble)
    val = np.polynomial.polynomial.polyval(lam, q)
    tm = np.cosh(order * np.arccosh(theta / delta))
    assert np.abs(val).max() <= (1.0 + 1e-12) / tm
    assert abs(np.abs(val).max() - 1.0 / tm) <= 1e-12 / tm  # attained at the ends
    assert abs(q[0] - 1.0) <= 1e-15  # q(0) = 1: the polynomial is consistent


def test_gershgorin_bounds_the_spectrum():
    for A in (_spd(40, 1), _spd(60, 2, 0.1), laplace(5)):
        d = A.diagonal()
        ev = scipy.linalg.eigvalsh((sp.diags(d ** -0.5) @ A @ sp.diags(d ** -0.5)).toarray())
        lo, hi = cheby_ref.gershgorin(A)
        assert lo == 0.0 and hi >= ev[-1]


def test_cg_with_n_steps_reproduces_the_extreme_eigenvalues():
    A = _spd(30, 7)
    d = A.diagonal()
    ev = scipy.linalg.eigvalsh((sp.diags(d ** -0.5) @ A @ sp.diags(d ** -0.5)).toarray())
    lo, hi, m = cheby_ref.cg_lanczos(A, 30)
    assert m <= 30
    assert abs(hi - ev[-1]) <= 1e-8 * ev[-1] and abs(lo - ev[0]) <= 1e-8 * ev[-1]
    # and a short run lies inside the spectrum: the estimate is from below / above
    lo10, hi10, m10 = cheby_ref.cg_lanczos(A, 10)
    assert m10 == 10 and ev[0] - 1e-12 <= lo10 <= hi10 <= ev[-1] + 1e-12


# Largest relative gap of lambda_min / lambda_max between the float64 and the longdouble CG-Lanczos of the restatement
# after 10 steps, level 0 of the operators the GPU test uses, measured 2026-10-19:
#   7-point 12^3: 2.84e-15 (lambda_min), 3.52e-16 (lambda_max);  27-point 10^3: 1.36e-15 (lambda_min), 3.35e-16 (lambda_max)
# tests/test_gpu_cheby.py takes 100 x the largest of these, and no less than 1e-13, for the device's estimate.  Reference
# against reference: what is asserted here is only that the gap stays below that floor (ten CG steps lose a few dozen
# roundings of 1.1e-16, not more).
REF_GAP = 2.84e-15


@pytest.mark.parametrize("n,stencil", [(12, 7), (10, 27)])
def test_float64_estimate_against_longdouble(n, stencil):
    A = laplace(n, stencil)
    lo, hi, m = cheby_ref.cg_lanczos(A, 10)
    lo_l, hi_l, m_l = cheby_ref.cg_lanczos(A, 10, dtype=np.longdouble)
    assert m == m_l == 10
    gaps = abs(lo - lo_l) / lo_l, abs(hi - hi_l) / hi_l
    print(f"{stencil}-point {n}^3: relative gap lambda_min {gaps[0]:.2e}, lambda_max {gaps[1]:.2e}")
    assert max(gaps) <= 1e-13, gaps


XC = {(2048, "fp64"): "spmv_stream_xc<2, 0, false, 256>", (2048, "dict"): "spmv_stream_xc<2, 0, true, 256>",
      (2048, "fp32"): "spmv_stream_xc<2, 0, false, 256, true>", (4096, "fp64"): "spmv_stream_xc<2, 0, false, 512>",
      (4096, "dict"): "spmv_stream_xc<2, 0, true, 512>", (4096, "fp32"): "spmv_stream_xc<2, 0, false, 512, true>"}
PLAIN = {"fp64": "spmv_stream<2, 0>", "dict": "spmv_stream<2, 0>", "fp32": "spmv_stream<2, 0, float>"}
HELD = {"fp64": dict(), "dict": dict(dictionary=True), "fp32": dict(fp32=True)}


def test_cheby_kernel_choice_table(mi_lib):
    for tile in (2048, 4096):
        for held, kw in HELD.items():
            assert mi_lib.cheby_kernel_choice(xcache=True, tile_entries=tile, **kw) == XC[(tile, held)]
            assert mi_lib.cheby_kernel_choice(xcache=False, tile_entries=tile, **kw) == PLAIN[held]
    # floats win over a dictionary, as for the other epilogues
    assert mi_lib.cheby_kernel_choice(xcache=True, fp32=True, dictionary=True) == XC[(2048, "fp32")]
    with pytest.raises(mi_lib.HypreError, match="tile_entries"):
        mi_lib.cheby_kernel_choice(tile_entries=1024)
    mi_lib.call("HYPRE_ClearAllErrors")


def test_solve_kernel_choice_still_refuses_the_third_epilogue(mi_lib):
    with pytest.raises(mi_lib.HypreError, match="epilogue"):
        mi_lib.solve_kernel_choice(0, epilogue=2)
    mi_lib.call("HYPRE_ClearAllErrors")


def test_new_symbols_are_exported(mi_lib):
    lib = mi_lib.lib()
    for name in ("HYPRE_BoomerAMGSetChebyOrder", "HYPRE_BoomerAMGSetChebyFraction", "HYPRE_BoomerAMGSetChebyEigEst",
                 "HYPRE_BoomerAMGSetChebyVariant", "HYPRE_BoomerAMGSetChebyScale", "HYPRE_MI_BoomerAMGGetLevelCheby",
                 "HYPRE_MI_ChebyKernelChoice"):
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr), name


def test_host_only_setup_says_why_it_refuses(mi_lib):
    mi = mi_lib
    A, rhs = mi.build_laplace_system_host(6, 6, 6, 7, 0, 1)
    amg = mi.BoomerAMG(print_level=0, relax_type=16)
    with pytest.raises(mi.HypreError, match="not implemented by the host-only setup.*no eigenvalue estimate"):
        mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
    mi.call("HYPRE_ClearAllErrors")
    amg = mi.BoomerAMG(print_level=0, relax_type=8, cheby_order=9)  # not type 16: the setting is not looked at
    mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
    assert amg.num_levels >= 2
