"""Parity of the GMRES + BoomerAMG path (setup, relaxation, V-cycle, Krylov loop)
against the CPU oracle on the same seeded inputs, through the C ABI.

Tolerances (fp64):
  * hierarchy: C/F splitting identical; P and the Galerkin operators agree to
    1e-14 relative (the host setup follows the oracle's loop order);
  * one relaxation call / one V-cycle: 1e-12 relative to max|u| (FMA contraction
    and reduction order differ between the HIP kernels and the oracle);
  * GMRES: same iteration count, residual history equal to 1e-8 relative per
    step, final relative residual equal within 1e-10 (the north-star bar),
    solution within the reference's own closeness rule rtol 1e-6 / atol 1e-8
    (/root/reference/src/HypreSystem.cpp:815-818) of both the oracle and x* = 1.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _chunk(mi):
    c = mi.c_int()
    mi.call("HYPRE_MI_GetGSChunk", mi.C.byref(c))
    return c.value


def _setup(mi, oc, n, stencil=7, **amg_kw):
    A, b, x, rhs = mi.build_laplace_system(n, n, n, stencil)
    amg = mi.BoomerAMG(print_level=0, **amg_kw)
    amg.setup(A)
    Ao, bo = oc.Csr.laplace(n, n, n, stencil)
    okw = dict(gs_chunk=_chunk(mi))
    if "relax_type" in amg_kw:
        okw["relax_type"] = amg_kw["relax_type"]
    if "num_sweeps" in amg_kw:
        okw["num_sweeps"] = amg_kw["num_sweeps"]
    for k in ("interp_type", "relax_order", "max_coarse_size", "strong_threshold", "cycle_type", "max_levels",
              "coarsen_type", "agg_num_levels", "agg_pmax_elmts", "agg_trunc_factor", "smooth_type",
              "smooth_num_levels", "ilu_max_iter", "ilu_tri_solve", "non_galerkin_tol", "ilu_level"):
        if k in amg_kw:
            okw[k] = amg_kw[k]
    for k, ok in (("ilu_lower_jacobi_iters", "ilu_lower_it"), ("ilu_upper_jacobi_iters", "ilu_upper_it")):
        if k in amg_kw:
            okw[ok] = amg_kw[k]
    oamg = oc.Amg(Ao, oc.default_params(**okw))
    return A, b, x, amg, Ao, bo, oamg


@pytest.mark.parametrize("n,stencil,interp", [(12, 7, 6), (20, 7, 6), (10, 27, 6), (16, 7, 3), (16, 7, 0)])
def test_hierarchy_matches_oracle(mi, oc, n, stencil, interp):
    A, b, x, amg, Ao, bo, oamg = _setup(mi, oc, n, stencil, interp_type=interp)
    assert amg.num_levels == oamg.num_levels
    for l in range(amg.num_levels):
        ia, ja, a, shape = amg.level_csr(l, 0)
        oia, oja, oa = oamg.level_A(l).arrays()
        assert shape == oamg.level_A(l).shape
        assert np.array_equal(ia, oia) and np.array_equal(ja, oja)
        assert np.allclose(a, oa, rtol=1e-14, atol=1e-14)
        if l < amg.num_levels - 1:
            assert np.array_equal(amg.level_cf(l), oamg.level_cf(l))
            pia, pja, pa, pshape = amg.level_csr(l, 2)
            qia, qja, qa = oamg.level_P(l).arrays()
            assert np.array_equal(pia, qia) and np.array_equal(pja, qja)
            assert np.allclose(pa, qa, rtol=1e-14, atol=1e-14)


@pytest.mark.parametrize("rtype", [0, 7, 18, 3, 4, 6, 8, 13, 14])
@pytest.mark.parametrize("points", [0, 1, -1])
def test_relax_matches_oracle(mi, oc, rtype, points):
    A, b, x, amg, Ao, bo, oamg = _setup(mi, oc, 14)
    rng = np.random.default_rng(100 + rtype)
    for level in (0, 1):
        nl = oamg.level_A(level).shape[0]
        f, u0 = rng.standard_normal(nl), rng.standard_normal(nl)
        got = amg.relax_level(level, rtype, points, f, u0)
        ref = oamg.relax(level, rtype, points, f, u0)
        assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
        if points != 0:
            cf = oamg.level_cf(level)
            assert np.array_equal(got[cf != points], u0[cf != points])


@pytest.mark.parametrize("rtype", [11, 12])
def test_two_stage_gauss_seidel_matches_oracle(mi, oc, rtype):
    """Relax types 11 / 12 (two-stage Gauss-Seidel: 1 / 2 Neumann terms for the forward solve): one call on two levels;
    the routine ignores the C/F marker, so every point moves whatever `points` says."""
    A, b, x, amg, Ao, bo, oamg = _setup(mi, oc, 14)
    rng = np.random.default_rng(200 + rtype)
    for level in (0, 1):
        nl = oamg.level_A(level).shape[0]
        f, u0 = rng.standard_normal(nl), rng.standard_normal(nl)
        for points in (0, 1):
            got = amg.relax_level(level, rtype, points, f, u0)
            ref = oamg.relax(level, rtype, points, f, u0)
            assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
            assert np.all(got != u0)


@pytest.mark.parametrize("density,longrow", [(0.004, None), (0.02, None), (0.05, (40, 1500)), (0.12, None)])
def test_relax_irregular_rows(mi, oc, density, longrow):
    """Ragged / long rows: every lanes-per-chunk variant of the cooperative GS kernel and its
    beyond-the-strip path, plus the Jacobi epilogue, against the oracle on level 0."""
    import scipy.sparse as sp

    n = 2000
    rng = np.random.default_rng(int(density * 1000))
    M = sp.random(n, n, density=density, random_state=rng, format="lil")
    if longrow:
        for c in rng.choice(n, size=longrow[1], replace=False):
            M[longrow[0], c] = rng.standard_normal()
    M = M.tocsr()
    M.setdiag(0.0)
    M.eliminate_zeros()
    M = -abs(M)  # M-matrix: negative couplings, weakly dominant diagonal
    M = (M + sp.diags(np.abs(M).sum(axis=1).A1 * 1.01 + 1e-3)).tocsr()
    M.sort_indices()
    A = mi.IJMatrix(0, n - 1)
    coo = M.tocoo()
    A.set_values_coo(coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data)
    A.assemble()
    amg = mi.BoomerAMG(print_level=0)
    amg.setup(A)
    oamg = oc.Amg(oc.Csr.from_scipy(M), oc.default_params(gs_chunk=_chunk(mi)))
    assert amg.num_levels == oamg.num_levels and amg.num_levels > 1
    assert np.array_equal(amg.level_cf(0), oamg.level_cf(0))
    f, u0 = rng.standard_normal(n), rng.standard_normal(n)
    for rtype in (8, 3, 14, 18):
        for points in (0, 1, -1):
            got = amg.relax_level(0, rtype, points, f, u0)
            ref = oamg.relax(0, rtype, points, f, u0)
            assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("coarsen", [8, 6, 0])
def test_gmres_amg_with_dirichlet_rows(mi, oc, coarsen):
    """Identity rows (Dirichlet boundary values kept in the system, as application matrices have them) in a 3-D
    convection-diffusion operator: points without strong connections through setup, cycle and GMRES."""
    import scipy.sparse as sp

    n = 14
    N = n ** 3
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n))
    Cx = sp.diags([-0.4, 0.4], [-1, 0], shape=(n, n))
    I = sp.identity(n)
    M = (sp.kron(sp.kron(I, I), T + Cx) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(T, I), I)).tolil()
    rng = np.random.default_rng(77)
    fixed = np.sort(rng.choice(N, size=N // 9, replace=False))
    for i in fixed:
        M.rows[i] = [int(i)]
        M.data[i] = [1.0]
    M = M.tocsr()
    M.sort_indices()
    xs = rng.standard_normal(N)
    bv = M @ xs
    A = mi.IJMatrix(0, N - 1)
    coo = M.tocoo()
    A.set_values_coo(coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data)
    A.assemble()
    b = mi.IJVector(0, N - 1, bv)
    x = mi.IJVector(0, N - 1, np.zeros(N))
    amg = mi.BoomerAMG(print_level=0, coarsen_type=coarsen)
    gm = mi.GMRES(tolerance=1e-9, max_iterations=100, kspace=40, print_level=0)
    gm.set_precond(amg)
    gm.setup(A, b, x)
    assert gm.solve(A, b, x) == 0
    Ao = oc.Csr.from_scipy(M)
    oamg = oc.Amg(Ao, oc.default_params(gs_chunk=_chunk(mi), coarsen_type=coarsen))
    assert amg.num_levels == oamg.num_levels
    cf = oamg.level_cf(0)  # in the level's C-first order
    assert np.array_equal(amg.level_cf(0), cf)
    if coarsen == 8:  # PMIS: a row without strong connections is a "special" F point, never a C point
        cf_nat = np.empty_like(cf)
        cf_nat[oamg.level_perm(0)] = cf
        assert np.all(cf_nat[fixed] != 1)
    xo, info = oc.gmres(Ao, bv, kdim=40, tol=1e-9, maxit=100, amg=oamg)
    assert gm.num_iterations == info["iters"]
    assert np.allclose(gm.residual_history(), info["norms"], rtol=1e-8, atol=1e-14 * info["norms"][0])
    assert _allclose_ref(x.get(), xs, rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("chunk", [1, 4, 16])
def test_relax_other_chunk_sizes(mi, oc, chunk):
    """Chunk sizes other than 8 take the generic lane-per-chunk kernel."""
    old = _chunk(mi)
    mi.call("HYPRE_MI_SetGSChunk", chunk)
    try:
        A, b, x, amg, Ao, bo, oamg = _setup(mi, oc, 12)
        rng = np.random.default_rng(chunk)
        f, u0 = rng.standard_normal(12 ** 3), rng.standard_normal(12 ** 3)
        for points in (0, 1, -1):
            got = amg.relax_level(0, 8, points, f, u0)
            ref = oamg.relax(0, 8, points, f, u0)
            assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    finally:
        mi.call("HYPRE_MI_SetGSChunk", old)


@pytest.mark.parametrize("kw", [dict(), dict(relax_type=18), dict(relax_type=6, num_sweeps=2, interp_type=0),
                                dict(relax_order=0), dict(cycle_type=2), dict(max_coarse_size=200),
                                # the upstream sample's AMG block (Falgout, classical interpolation, SGS, 2 sweeps)
                                dict(coarsen_type=6, relax_type=6, num_sweeps=2, interp_type=0),
                                dict(coarsen_type=10), dict(agg_num_levels=1), dict(agg_num_levels=2, cycle_type=2),
                                dict(interp_type=4),  # multipass interpolation on ordinary splittings
                                dict(coarsen_type=0), dict(coarsen_type=7, max_levels=6),  # CLJP
                                dict(relax_type=11, relax_order=0, num_sweeps=2), dict(relax_type=12),  # two-stage GS
                                # complex smoother (src/HypreSystem.cpp:235-320): ILU(0) on the finest level(s)
                                dict(smooth_type=5, smooth_num_levels=1), dict(smooth_type=5, smooth_num_levels=3, num_sweeps=2),
                                dict(smooth_type=5, smooth_num_levels=2, ilu_max_iter=2, cycle_type=2),
                                dict(smooth_type=5, smooth_num_levels=2, ilu_tri_solve=0, ilu_lower_jacobi_iters=3,
                                     ilu_upper_jacobi_iters=4),
                                dict(smooth_type=5, smooth_num_levels=2, ilu_level=1),  # ILU(1) as the complex smoother
                                dict(smooth_type=5, smooth_num_levels=50)])
def test_vcycle_matches_oracle(mi, oc, kw):
    A, b, x, amg, Ao, bo, oamg = _setup(mi, oc, 16, **kw)
    rng = np.random.default_rng(7)
    f = rng.standard_normal(16 ** 3)
    fi = mi.IJVector(0, 16 ** 3 - 1, f)
    ui = mi.IJVector(0, 16 ** 3 - 1, np.zeros(16 ** 3))
    amg.solve(A, fi, ui)  # max_iterations 1, tolerance 0: exactly one cycle
    got = ui.get()
    ref = oamg.cycle(f)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    # the cycle is a linear operator: M(a f) = a M(f)
    fi2 = mi.IJVector(0, 16 ** 3 - 1, -2.5 * f)
    ui2 = mi.IJVector(0, 16 ** 3 - 1, np.zeros(16 ** 3))
    amg.solve(A, fi2, ui2)
    assert np.abs(ui2.get() + 2.5 * got).max() <= 1e-12 * np.abs(got).max() * 2.5


def _allclose_ref(x, xref, rtol=1e-6, atol=1e-8):
    """check_solution's rule, /root/reference/src/HypreSystem.cpp:815-818."""
    diff = np.abs(x - xref)
    return np.all(diff < np.maximum(rtol * np.maximum(np.abs(x), np.abs(xref)), atol))


@pytest.mark.parametrize("n,stencil", [(16, 7), (10, 27)])
def test_zero_guess_sub_operator(mi, n, stencil):
    """The first sweep of every down leg starts from u = 0 and runs on the level's zero-guess sub-operator (rows'
    in-chunk entries + the F rows' C columns; everything else multiplies zeros): the operator has exactly those
    entries, and the solve agrees with the one that sweeps the full operator (mode 0) up to summation order.  Mode 3
    adds the residual operator that follows the sweep."""
    runs = {}
    try:
        for mode in (0, 1, 2, 3):
            mi.call("HYPRE_MI_SetZeroGuessMode", mode)
            A, b, x, rhs = mi.build_laplace_system(n, n, n, stencil)
            amg = mi.BoomerAMG(print_level=0)
            gm = mi.GMRES(tolerance=1e-10, max_iterations=100, kspace=50, print_level=0)
            gm.set_precond(amg)
            gm.setup(A, b, x)
            assert gm.solve(A, b, x) == 0
            runs[mode] = (gm.num_iterations, np.asarray(gm.residual_history()), x.get())
            checked = 0
            for l in range(amg.num_levels - 1):
                nr, nc_, nnz = mi.c_int(), mi.c_int(), mi.C.c_longlong()
                mi.call("HYPRE_MI_BoomerAMGGetLevelCSRSize", amg.h, l, 6, mi.C.byref(nr), mi.C.byref(nc_), mi.C.byref(nnz))
                if mode < 2:
                    assert nr.value == 0 and nnz.value == 0
                    continue
                ia, ja, a, shape = amg.level_csr(l, 0)
                ncoarse = int((np.asarray(amg.level_cf(l)) == 1).sum())
                rows = np.repeat(np.arange(shape[0]), np.diff(ia))
                keep = (ja // 8 == rows // 8) | ((rows >= ncoarse) & (ja < ncoarse))
                assert nr.value == shape[0] and nnz.value == int(keep.sum()) and nnz.value < len(ja)
                # mode 3: the operator of the residual after that sweep -- F rows from the first chunk boundary
                # >= nc on without their C columns (the F pass hands their product over)
                mi.call("HYPRE_MI_BoomerAMGGetLevelCSRSize", amg.h, l, 8, mi.C.byref(nr), mi.C.byref(nc_), mi.C.byref(nnz))
                if mode == 3:
                    t_from = (ncoarse + 7) // 8 * 8
                    dropped = (rows >= t_from) & (ja < ncoarse)
                    assert nr.value == shape[0] and nnz.value == len(ja) - int(dropped.sum())
                    assert l > 1 or dropped.any()
                else:
                    assert nr.value == 0 and nnz.value == 0
                checked += 1
            assert mode < 2 or checked >= 2
    finally:
        mi.call("HYPRE_MI_SetZeroGuessMode", 3)
    for mode in (1, 2, 3):
        assert runs[mode][0] == runs[0][0]
        assert np.allclose(runs[mode][1], runs[0][1], rtol=1e-9, atol=0.0)
        assert np.abs(runs[mode][2] - runs[0][2]).max() <= 1e-12


@pytest.mark.parametrize("n,stencil,kdim,tol", [(16, 7, 50, 1e-8), (24, 7, 5, 1e-10), (12, 27, 50, 1e-8),
                                                  (32, 7, 50, 1e-6)])
def test_gmres_amg_matches_oracle(mi, oc, n, stencil, kdim, tol):
    A, b, x, amg, Ao, bo, oamg = _setup(mi, oc, n, stencil)
    gm = mi.GMRES(tolerance=tol, max_iterations=100, kspace=kdim, print_level=0)
    gm.set_precond(amg)
    gm.setup(A, b, x)
    rc = gm.solve(A, b, x)
    assert rc == 0
    xo, info = oc.gmres(Ao, bo, kdim=kdim, tol=tol, maxit=100, amg=oamg)
    assert gm.num_iterations == info["iters"]
    hist = gm.residual_history()
    assert len(hist) == len(info["norms"])
    assert np.allclose(hist, info["norms"], rtol=1e-8, atol=0.0)
    assert abs(gm.final_rel_res - info["rel_res"]) <= 1e-10
    xs = x.get()
    assert _allclose_ref(xs, xo)
    assert _allclose_ref(xs, np.ones_like(xs), rtol=max(1e-6, 100 * tol))
    # true residual of the device solution, computed by the oracle's SpMV
    r = bo - Ao.matvec(xs)
    assert np.linalg.norm(r) / np.linalg.norm(bo) <= tol * 1.0000001


@pytest.mark.parametrize("kw", [dict(coarsen_type=6, relax_type=6, num_sweeps=2, interp_type=0), dict(coarsen_type=10),
                                dict(agg_num_levels=1), dict(agg_num_levels=1, agg_pmax_elmts=4, coarsen_type=10),
                                dict(smooth_type=5, smooth_num_levels=2),
                                dict(non_galerkin_tol=0.05)])  # non-Galerkin coarse operators, HypreSystem.cpp:161-176
def test_gmres_amg_other_hierarchies_match_oracle(mi, oc, kw):
    """GMRES behind the other coarsening choices (src/HypreSystem.cpp:125-126, :215-229): same bars as above."""
    n = 20
    A, b, x, amg, Ao, bo, oamg = _setup(mi, oc, n, 7, **kw)
    gm = mi.GMRES(tolerance=1e-9, max_iterations=100, kspace=30, print_level=0)
    gm.set_precond(amg)
    gm.setup(A, b, x)
    assert gm.solve(A, b, x) == 0
    xo, info = oc.gmres(Ao, bo, kdim=30, tol=1e-9, maxit=100, amg=oamg)
    assert gm.num_iterations == info["iters"]
    # 1e-8 per step, above a rounding floor of 1e-14 of the initial residual (the ILU substitutions of the complex
    # smoother sum in another order on the device; ten orders of reduction amplify that in the last step)
    assert np.allclose(gm.residual_history(), info["norms"], rtol=1e-8, atol=1e-14 * info["norms"][0])
    assert abs(gm.final_rel_res - info["rel_res"]) <= 1e-10
    assert _allclose_ref(x.get(), xo) and _allclose_ref(x.get(), np.ones(n ** 3))


def test_gmres_no_precond_and_restart(mi, oc):
    """Restarted GMRES(7) without a preconditioner (several restart cycles, residual vector rebuilt from the
    Givens data).  Unpreconditioned restarts amplify rounding differences between the two implementations
    (FMA contraction, reduction order) by orders of magnitude over tens of cycles, so the history is compared
    tightly over the first cycles and loosely afterwards; the end state is checked on its own."""
    n = 10
    A, b, x, rhs = mi.build_laplace_system(n, n, n, 7)
    gm = mi.GMRES(tolerance=1e-7, max_iterations=200, kspace=7, print_level=0)
    gm.setup(A, b, x)
    assert gm.solve(A, b, x) == 0
    Ao, bo = oc.Csr.laplace(n, n, n, 7)
    xo, info = oc.gmres(Ao, bo, kdim=7, tol=1e-7, maxit=200, amg=None)
    assert abs(gm.num_iterations - info["iters"]) <= 1 and gm.num_iterations > 3 * 7
    hist, ref = gm.residual_history(), info["norms"]
    m = min(len(hist), len(ref))
    assert np.allclose(hist[:22], ref[:22], rtol=1e-9)       # three full restart cycles
    assert np.allclose(hist[:m], ref[:m], rtol=0.05)
    assert _allclose_ref(x.get(), xo, rtol=1e-5)
    r = bo - Ao.matvec(x.get())
    assert np.linalg.norm(r) <= 1e-7 * np.linalg.norm(bo) * 1.000001


def test_gmres_maxiter_reports_conv_error(mi):
    n = 12
    A, b, x, rhs = mi.build_laplace_system(n, n, n, 7)
    gm = mi.GMRES(tolerance=1e-14, max_iterations=3, kspace=50, print_level=0)
    gm.setup(A, b, x)
    assert gm.solve(A, b, x) == mi.HYPRE_ERROR_CONV
    assert gm.num_iterations == 3
    mi.call("HYPRE_ClearAllErrors")


def test_bicgstab_amg_matches_oracle(mi, oc):
    A, b, x, amg, Ao, bo, oamg = _setup(mi, oc, 16)
    bi = mi.BiCGSTAB(tolerance=1e-8, max_iterations=50, print_level=0)
    bi.set_precond(amg)
    bi.setup(A, b, x)
    assert bi.solve(A, b, x) == 0
    xo, info = oc.bicgstab(Ao, bo, tol=1e-8, maxit=50, amg=oamg)
    assert bi.num_iterations == info["iters"]
    assert abs(bi.final_rel_res - info["rel_res"]) <= 1e-10
    assert _allclose_ref(x.get(), xo)


@pytest.mark.parametrize("kdim", [50, 4])
def test_flexgmres_amg_matches_oracle(mi, oc, kdim):
    A, b, x, amg, Ao, bo, oamg = _setup(mi, oc, 16)
    fg = mi.FlexGMRES(tolerance=1e-9, max_iterations=60, kspace=kdim, print_level=0)
    fg.set_precond(amg)
    fg.setup(A, b, x)
    assert fg.solve(A, b, x) == 0
    xo, info = oc.fgmres(Ao, bo, kdim=kdim, tol=1e-9, maxit=60, amg=oamg)
    assert fg.num_iterations == info["iters"]
    assert np.allclose(fg.residual_history(), info["norms"], rtol=1e-7)
    assert abs(fg.final_rel_res - info["rel_res"]) <= 1e-10
    assert _allclose_ref(x.get(), xo)


@pytest.mark.parametrize("kdim,cgs", [(50, 0), (12, 0), (50, 2), (5, 2)])
def test_cogmres_amg_matches_oracle(mi, oc, kdim, cgs):
    """GMRES skeleton with classical Gram-Schmidt in block form (one block of inner products + one block
    update per pass; kdim 12 crosses the 8-vector block of the kernels, kdim 5 restarts)."""
    A, b, x, amg, Ao, bo, oamg = _setup(mi, oc, 16)
    cg = mi.COGMRES(tolerance=1e-9, max_iterations=60, kspace=kdim, print_level=0)
    mi.call("HYPRE_ParCSRCOGMRESSetCGS", cg.h, cgs)
    cg.set_precond(amg)
    cg.setup(A, b, x)
    assert cg.solve(A, b, x) == 0
    xo, info = oc.cogmres(Ao, bo, kdim=kdim, cgs=cgs, tol=1e-9, maxit=60, amg=oamg)
    assert cg.num_iterations == info["iters"]
    assert np.allclose(cg.residual_history(), info["norms"], rtol=1e-6)
    assert abs(cg.final_rel_res - info["rel_res"]) <= 1e-10
    assert _allclose_ref(x.get(), xo)
    # same Krylov space as GMRES: the counts agree while orthogonality holds
    _, ginfo = oc.gmres(Ao, bo, kdim=kdim, tol=1e-9, maxit=60, amg=oamg)
    assert abs(info["iters"] - ginfo["iters"]) <= 1


@pytest.mark.parametrize("precond", [True, False])
def test_pcg_matches_oracle(mi, oc, precond):
    A, b, x, amg, Ao, bo, oamg = _setup(mi, oc, 14)
    cg = mi.PCG(tolerance=1e-9, max_iterations=200, print_level=0)
    if precond:
        cg.set_precond(amg)
    cg.setup(A, b, x)
    assert cg.solve(A, b, x) == 0
    xo, info = oc.pcg(Ao, bo, tol=1e-9, maxit=200, amg=oamg if precond else None)
    assert cg.num_iterations == info["iters"]
    assert np.allclose(cg.residual_history(), info["norms"], rtol=1e-6)
    assert _allclose_ref(x.get(), xo) and _allclose_ref(x.get(), np.ones(14 ** 3), rtol=1e-6)


def test_against_direct_solve(mi):
    """Independent known answer: scipy's sparse direct solve of a non-symmetric system."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl

    rng = np.random.default_rng(42)
    n = 3000
    M = sp.random(n, n, density=0.002, random_state=rng, format="csr")
    M = (M - sp.diags(M.diagonal())).tocsr()
    M = (-abs(M) + sp.diags(abs(M).sum(axis=1).A1 + 0.5)).tocsr()
    M.sort_indices()
    xstar = rng.standard_normal(n)
    rhs = M @ xstar
    A = mi.IJMatrix(0, n - 1)
    coo = M.tocoo()
    A.set_values_coo(coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data)
    A.assemble()
    b = mi.IJVector(0, n - 1, rhs)
    x = mi.IJVector(0, n - 1, np.zeros(n))
    amg = mi.BoomerAMG(print_level=0)
    gm = mi.GMRES(tolerance=1e-12, max_iterations=200, kspace=50, print_level=0)
    gm.set_precond(amg)
    gm.setup(A, b, x)
    assert gm.solve(A, b, x) == 0
    xd = spl.spsolve(M.tocsc(), rhs)
    assert np.abs(x.get() - xd).max() <= 1e-8 * np.abs(xd).max()


@pytest.mark.parametrize("n,stencil,trisolve", [(12, 7, 1), (9, 27, 1), (12, 7, 0)])
def test_ilu0_matches_oracle(mi, oc, n, stencil, trisolve):
    """HYPRE_ILU type 0 / fill 0: application, GMRES preconditioning and the Richardson solver against the oracle.
    The device factorisation and substitutions repeat the oracle's operation order (no FMA): applications agree
    to rounding of the final division only."""
    A, b, x, rhs = mi.build_laplace_system(n, n, n, stencil)
    Ao, bo = oc.Csr.laplace(n, n, n, stencil)
    ilu = mi.ILU(max_iterations=1, tolerance=0.0, trisolve=trisolve, lower_jacobi_iters=4, upper_jacobi_iters=3)
    oilu = oc.Ilu(Ao, tri_solve=trisolve, lower_it=4, upper_it=3)
    ilu.setup(A)
    # one application on a zero guess: x = M^-1 b (through the solver entry point)
    rng = np.random.default_rng(4)
    v = rng.standard_normal(n ** 3)
    bv = mi.IJVector(0, n ** 3 - 1, v)
    xv = mi.IJVector(0, n ** 3 - 1, np.zeros(n ** 3))
    ilu.solve(A, bv, xv)
    ref = oilu.apply(v)
    assert np.allclose(xv.get(), ref, rtol=1e-13, atol=1e-13 * np.abs(ref).max())
    # as the preconditioner of GMRES
    gm = mi.GMRES(tolerance=1e-9, max_iterations=200, kspace=40, print_level=0)
    gm.set_precond(ilu)
    gm.setup(A, b, x)
    assert gm.solve(A, b, x) == 0
    xo, info = oc.gmres(Ao, bo, kdim=40, tol=1e-9, maxit=200, amg=oilu)
    assert gm.num_iterations == info["iters"]
    assert np.allclose(gm.residual_history(), info["norms"], rtol=1e-7)
    assert _allclose_ref(x.get(), xo)
    # as a solver: Richardson iteration to a tolerance
    if trisolve:
        sol = mi.ILU(max_iterations=300, tolerance=1e-6)
        sol.setup(A)
        x.fill(0.0)
        sol.solve(A, b, x)
        xs, si = oilu.solve(bo, max_iter=300, tol=1e-6)
        assert sol.num_iterations == si["iters"] and _allclose_ref(x.get(), xs)


def test_ilu_unsupported_variants_report_errors(mi):
    A, b, x, rhs = mi.build_laplace_system(6, 6, 6, 7)
    ilu = mi.ILU(ilu_type=1)
    with pytest.raises(mi.HypreError):
        ilu.setup(A)
    mi.call("HYPRE_ClearAllErrors")
    ilu = mi.ILU(fill=-1)
    with pytest.raises(mi.HypreError):
        ilu.setup(A)
    mi.call("HYPRE_ClearAllErrors")


@pytest.mark.parametrize("n,stencil,fill,trisolve", [(12, 7, 1, 1), (10, 7, 2, 1), (8, 27, 1, 1), (12, 7, 2, 0)])
def test_iluk_matches_oracle(mi, oc, n, stencil, fill, trisolve):
    """HYPRE_ILU type 0 with level of fill k (HYPRE_ILUSetLevelOfFill, /root/reference/src/HypreSystem.cpp:345-349): the
    symbolic pattern is built on the host, the numeric factorisation and the substitutions are the ILU(0) kernels on
    that pattern -- application, GMRES preconditioning (fewer iterations than ILU(0)) against the oracle."""
    A, b, x, rhs = mi.build_laplace_system(n, n, n, stencil)
    Ao, bo = oc.Csr.laplace(n, n, n, stencil)
    ilu = mi.ILU(max_iterations=1, tolerance=0.0, trisolve=trisolve, lower_jacobi_iters=6, upper_jacobi_iters=6, fill=fill)
    oilu = oc.Ilu(Ao, tri_solve=trisolve, lower_it=6, upper_it=6, level_of_fill=fill)
    ilu.setup(A)
    rng = np.random.default_rng(40 + fill)
    v = rng.standard_normal(n ** 3)
    bv = mi.IJVector(0, n ** 3 - 1, v)
    xv = mi.IJVector(0, n ** 3 - 1, np.zeros(n ** 3))
    ilu.solve(A, bv, xv)
    ref = oilu.apply(v)
    assert np.allclose(xv.get(), ref, rtol=1e-13, atol=1e-13 * np.abs(ref).max())
    gm = mi.GMRES(tolerance=1e-9, max_iterations=200, kspace=40, print_level=0)
    gm.set_precond(ilu)
    gm.setup(A, b, x)
    assert gm.solve(A, b, x) == 0
    xo, info = oc.gmres(Ao, bo, kdim=40, tol=1e-9, maxit=200, amg=oilu)
    assert gm.num_iterations == info["iters"]
    assert np.allclose(gm.residual_history(), info["norms"], rtol=1e-7)
    assert _allclose_ref(x.get(), xo)
    if trisolve:
        x0, info0 = oc.gmres(Ao, bo, kdim=40, tol=1e-9, maxit=200, amg=oc.Ilu(Ao))
        assert info["iters"] < info0["iters"]


def _ij_from_scipy(mi, M):
    M = M.tocsr()
    A = mi.IJMatrix(0, M.shape[0] - 1)
    coo = M.tocoo()
    A.set_values_coo(coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data.astype(np.float64))
    A.assemble()
    return A


@pytest.mark.parametrize("case", ["one_by_one", "diagonal", "zero_rhs", "tiny_dense"])
def test_degenerate_systems(mi, case):
    """Edge cases of the solve path: a 1x1 system, a diagonal operator (empty strength graph: single level),
    a zero right-hand side (zero iterations, x = 0), a small dense block (coarsest-level direct solve only)."""
    import scipy.sparse as sp

    rng = np.random.default_rng(8)
    if case == "one_by_one":
        M, rhs = sp.csr_matrix(np.array([[4.0]])), np.array([2.0])
    elif case == "diagonal":
        d = 1.0 + rng.random(300)
        M, rhs = sp.diags(d).tocsr(), rng.standard_normal(300)
    elif case == "zero_rhs":
        T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(200, 200))
        M, rhs = T.tocsr(), np.zeros(200)
    else:
        B = rng.random((7, 7))
        M, rhs = sp.csr_matrix(B @ B.T + 7 * np.eye(7)), rng.standard_normal(7)
    n = M.shape[0]
    A = _ij_from_scipy(mi, M)
    b = mi.IJVector(0, n - 1, rhs)
    x = mi.IJVector(0, n - 1, np.zeros(n))
    amg = mi.BoomerAMG(print_level=0)
    gm = mi.GMRES(tolerance=1e-12, max_iterations=50, kspace=20, print_level=0)
    gm.set_precond(amg)
    gm.setup(A, b, x)
    assert gm.solve(A, b, x) == 0
    xs = x.get()
    if case == "zero_rhs":
        assert gm.num_iterations == 0 and np.all(xs == 0.0)
    else:
        ref = np.linalg.solve(M.toarray(), rhs)
        assert np.allclose(xs, ref, rtol=1e-9, atol=1e-12)
        assert gm.num_iterations <= 10
    if case in ("one_by_one", "diagonal", "tiny_dense"):
        assert amg.num_levels == 1


def test_unimplemented_complex_smoother_is_refused(mi):
    """smooth_num_levels > 0 with a smoother other than ILU (HYPRE's default smooth_type is 6 = Schwarz), or an ILU
    variant other than block-Jacobi ILU(k): Setup fails with HYPRE_ERROR_ARG instead of smoothing with something else."""
    A, b, x, rhs = mi.build_laplace_system(8, 8, 8, 7)
    for kw in (dict(smooth_num_levels=1), dict(smooth_type=6, smooth_num_levels=2),
               dict(smooth_type=5, smooth_num_levels=1, ilu_type=10), dict(smooth_type=5, smooth_num_levels=1, ilu_level=-1)):
        amg = mi.BoomerAMG(print_level=0, **kw)
        with pytest.raises(mi.HypreError) as e:
            amg.setup(A)
        assert "not implemented" in str(e.value)
    amg = mi.BoomerAMG(print_level=0, smooth_type=6)  # no levels: the type alone has no effect
    amg.setup(A)


def _combo(seed):
    """One seeded combination of the BoomerAMG choices this library implements."""
    rng = np.random.default_rng(1000 + seed)
    kw = dict(coarsen_type=int(rng.choice([8, 8, 10, 6, 0, 3])), interp_type=int(rng.choice([6, 6, 0, 3, 4])),
              relax_type=int(rng.choice([8, 8, 6, 3, 13, 18, 11, 7])), cycle_type=int(rng.choice([1, 1, 2])),
              num_sweeps=int(rng.choice([1, 1, 2])), relax_order=int(rng.choice([1, 1, 0])),
              strong_threshold=float(rng.choice([0.25, 0.5, 0.57])))
    if rng.random() < 0.3:
        kw["agg_num_levels"] = int(rng.choice([1, 2]))
    if rng.random() < 0.25:
        kw.update(smooth_type=5, smooth_num_levels=int(rng.choice([1, 2])))
    if rng.random() < 0.3:
        kw["max_coarse_size"] = int(rng.choice([40, 150]))
    # (round 3; its own stream so that the combinations above stay what they were) non-Galerkin coarse operators
    rng2 = np.random.default_rng(90000 + seed)
    if rng2.random() < 0.3:
        kw["non_galerkin_tol"] = float(rng2.choice([0.02, 0.05, 0.1]))
    return kw


@pytest.mark.parametrize("seed", range(int(__import__("os").environ.get("MI_TEST_COMBOS", "20"))))
def test_seeded_parameter_combinations_match_oracle(mi, oc, seed):
    """Interactions of the implemented BoomerAMG choices (coarsening x interpolation x smoother x cycle x aggressive
    levels x complex smoother) on a non-symmetric convection-diffusion operator: hierarchy, iteration count,
    residual history and solution against the oracle for 20 seeded combinations."""
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from systems import convection_diffusion_3d

    kw = _combo(seed)
    n = 13
    M = convection_diffusion_3d(n, seed=50 + seed)
    N = M.shape[0]
    rng = np.random.default_rng(seed)
    xs = rng.standard_normal(N)
    bv = M @ xs
    A = mi.matrix_from_scipy(M)
    b = mi.IJVector(0, N - 1, bv)
    x = mi.IJVector(0, N - 1, np.zeros(N))
    amg = mi.BoomerAMG(print_level=0, **kw)
    gm = mi.GMRES(tolerance=1e-8, max_iterations=80, kspace=30, print_level=0)
    gm.set_precond(amg)
    gm.setup(A, b, x)
    rc = gm.solve(A, b, x)
    Ao = oc.Csr.from_scipy(M)
    oamg = oc.Amg(Ao, oc.default_params(gs_chunk=_chunk(mi), **kw))
    xo, info = oc.gmres(Ao, bv, kdim=30, tol=1e-8, maxit=80, amg=oamg)
    assert amg.num_levels == oamg.num_levels, kw
    assert np.array_equal(amg.level_cf(0), oamg.level_cf(0)), kw
    assert gm.num_iterations == info["iters"], (kw, gm.num_iterations, info["iters"])
    assert np.allclose(gm.residual_history(), info["norms"], rtol=1e-7, atol=1e-13 * info["norms"][0]), kw
    if info["rel_res"] <= 1e-8:
        assert rc == 0 and _allclose_ref(x.get(), xs, rtol=1e-4, atol=1e-6), kw


@pytest.mark.parametrize("seed", range(int(__import__("os").environ.get("MI_TEST_RANDOM_SYSTEMS", "10"))))
def test_seeded_random_systems_match_oracle(mi, oc, seed):
    """Irregular graphs: seeded random M-matrices (5 to 250 entries per row -- narrow rows, rows longer than a chunk's
    share of a tile, the wide tiles), some with identity rows, under seeded combinations of the BoomerAMG choices:
    hierarchy, iterations, residual history and solution against the oracle."""
    import scipy.sparse as sp

    rng = np.random.default_rng(7000 + seed)
    n = int(rng.integers(400, 2600))
    per_row = float(rng.choice([5, 12, 30, 80, 150, 250]))
    M = sp.random(n, n, density=min(0.5, per_row / n), random_state=rng, format="csr")
    M = (M + M.T).tocsr() if rng.random() < 0.5 else M
    M = (M - sp.diags(M.diagonal())).tocsr()
    M.eliminate_zeros()
    M = (-abs(M) + sp.diags(abs(M).sum(axis=1).A1 * float(rng.choice([1.0, 1.02, 1.3])) + 1e-3)).tolil()
    if rng.random() < 0.4:
        for i in rng.choice(n, size=n // 12, replace=False):
            M.rows[i] = [int(i)]
            M.data[i] = [1.0]
    M = M.tocsr()
    M.sort_indices()
    kw = _combo(500 + seed)
    xs = rng.standard_normal(n)
    bv = M @ xs
    A = mi.matrix_from_scipy(M)
    b = mi.IJVector(0, n - 1, bv)
    x = mi.IJVector(0, n - 1, np.zeros(n))
    amg = mi.BoomerAMG(print_level=0, **kw)
    gm = mi.GMRES(tolerance=1e-8, max_iterations=60, kspace=30, print_level=0)
    gm.set_precond(amg)
    gm.setup(A, b, x)
    rc = gm.solve(A, b, x)
    Ao = oc.Csr.from_scipy(M)
    oamg = oc.Amg(Ao, oc.default_params(gs_chunk=_chunk(mi), **kw))
    xo, info = oc.gmres(Ao, bv, kdim=30, tol=1e-8, maxit=60, amg=oamg)
    what = (seed, n, per_row, kw)
    assert amg.num_levels == oamg.num_levels, what
    if amg.num_levels > 1:
        assert np.array_equal(amg.level_cf(0), oamg.level_cf(0)), what
    assert gm.num_iterations == info["iters"], (what, gm.num_iterations, info["iters"])
    hist, ref = np.asarray(gm.residual_history()), np.asarray(info["norms"])
    if info["rel_res"] <= 1e-8:  # converged: the whole history, and the solution against the oracle's
        assert rc == 0 and np.allclose(hist, ref, rtol=1e-7, atol=1e-13 * ref[0]), what
        assert _allclose_ref(x.get(), xo, rtol=1e-5, atol=1e-7), what
    else:
        # nearly singular draws under a smoother that does not converge on them stagnate (seed 130: identical
        # hierarchy, one cycle equal to 2e-14, yet the Arnoldi vectors cancel to ~1e-9 of their size and the
        # histories part in the third step): only the start is comparable, and both sides must have stalled
        assert np.allclose(hist[:2], ref[:2], rtol=1e-7, atol=0.0) and hist[-1] > 1e-8 * hist[0], what


@pytest.mark.parametrize("seed", range(int(__import__("os").environ.get("MI_TEST_SOLVER_COMBOS", "12"))))
def test_seeded_solver_families_match_oracle(mi, oc, seed):
    """The other Krylov families (src/HypreSystem.cpp:372-497: bicg, fgmres, cogmres, cg) behind seeded combinations of
    the BoomerAMG choices, on the non-symmetric convection-diffusion operator (cg: the 7-point Laplacian)."""
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from systems import convection_diffusion_3d

    rng = np.random.default_rng(9000 + seed)
    method = ["bicgstab", "fgmres", "cogmres", "pcg"][seed % 4]
    kw = _combo(800 + seed)
    n = int(rng.integers(10, 15))
    if method == "pcg":
        Ao, _ = oc.Csr.laplace(n, n, n, 7)
        M = Ao.to_scipy().tocsr()
        kw["relax_type"] = int(rng.choice([6, 8, 18, 7]))  # a symmetric smoother keeps the preconditioner SPD
        kw.pop("smooth_type", None), kw.pop("smooth_num_levels", None)
    else:
        M = convection_diffusion_3d(n, seed=300 + seed)
    N = M.shape[0]
    xs = rng.standard_normal(N)
    bv = M @ xs
    A = mi.matrix_from_scipy(M)
    b = mi.IJVector(0, N - 1, bv)
    x = mi.IJVector(0, N - 1, np.zeros(N))
    amg = mi.BoomerAMG(print_level=0, **kw)
    Ao = oc.Csr.from_scipy(M)
    oamg = oc.Amg(Ao, oc.default_params(gs_chunk=_chunk(mi), **kw))
    kdim = int(rng.choice([6, 20, 40]))
    if method == "bicgstab":
        s = mi.BiCGSTAB(tolerance=1e-8, max_iterations=60, print_level=0)
        xo, info = oc.bicgstab(Ao, bv, tol=1e-8, maxit=60, amg=oamg)
    elif method == "fgmres":
        s = mi.FlexGMRES(tolerance=1e-8, max_iterations=60, kspace=kdim, print_level=0)
        xo, info = oc.fgmres(Ao, bv, kdim=kdim, tol=1e-8, maxit=60, amg=oamg)
    elif method == "cogmres":
        s = mi.COGMRES(tolerance=1e-8, max_iterations=60, kspace=kdim, print_level=0)
        cgs = int(rng.choice([0, 2]))
        mi.call("HYPRE_ParCSRCOGMRESSetCGS", s.h, cgs)
        xo, info = oc.cogmres(Ao, bv, kdim=kdim, cgs=cgs, tol=1e-8, maxit=60, amg=oamg)
    else:
        s = mi.PCG(tolerance=1e-8, max_iterations=60, print_level=0)
        xo, info = oc.pcg(Ao, bv, tol=1e-8, maxit=60, amg=oamg)
    s.set_precond(amg)
    s.setup(A, b, x)
    rc = s.solve(A, b, x)
    what = (seed, method, n, kdim, kw)
    assert s.num_iterations == info["iters"], (what, s.num_iterations, info["iters"])
    if info["iters"] < 60:
        assert rc == 0 and abs(s.final_rel_res - info["rel_res"]) <= 1e-9, what
        assert _allclose_ref(x.get(), xo, rtol=1e-5, atol=1e-7), what


def test_zero_guess_cycles_never_read_the_vectors_they_do_not_fill(mi):
    """BoomerAMG::zero_cycle_ignores_u skips the zero-fill of a level's vector when the first sweep on the
    zero guess overwrites every row without reading it.  "Never read" is checked here: with every level's solution and
    scratch vectors poisoned with NaN before each solve, GMRES + BoomerAMG gives the bits it gives on clean vectors
    (7- and 27-point, with the collapsed dense tail in play on the coarse levels)."""
    for n, stencil in ((20, 7), (12, 27)):
        A, b, x, rhs = mi.build_laplace_system(n, n, n, stencil)
        amg = mi.BoomerAMG(print_level=0)
        gm = mi.GMRES(tolerance=1e-10, max_iterations=100, kspace=50, print_level=0)
        gm.set_precond(amg)
        gm.setup(A, b, x)
        assert gm.solve(A, b, x) == 0
        ref = (gm.num_iterations, np.asarray(gm.residual_history()).copy(), x.get().copy())
        assert amg.num_levels >= 3
        for _ in range(2):
            mi.call("HYPRE_MI_BoomerAMGPoisonWorkVectors", amg.h)
            x.fill(0.0)
            assert gm.solve(A, b, x) == 0
            xs = x.get()
            assert np.all(np.isfinite(xs))
            assert gm.num_iterations == ref[0] and np.array_equal(np.asarray(gm.residual_history()), ref[1])
            assert np.array_equal(xs, ref[2])


def test_cycle_setters_after_setup_reach_the_collapsed_tail(mi, oc):
    """the tabulated dense maps of the coarse tail were frozen at Setup, so a relax type or sweep count set
    AFTER Setup changed the fine levels' cycle only.  Now the maps are tabulated again when the cycle's parameters
    differ: a solver whose smoother is switched after Setup behaves exactly like one that was set up with it."""
    n = 20
    runs = []
    for late in (False, True):
        A, b, x, rhs = mi.build_laplace_system(n, n, n, 7)
        kw = {} if late else {"relax_type": 6, "num_sweeps": 2}
        amg = mi.BoomerAMG(print_level=0, **kw)
        gm = mi.GMRES(tolerance=1e-10, max_iterations=100, kspace=50, print_level=0)
        gm.set_precond(amg)
        gm.setup(A, b, x)
        if late:
            assert gm.solve(A, b, x) == 0  # (the default cycle first: its maps exist and must go)
            mi.call("HYPRE_BoomerAMGSetRelaxType", amg.h, 6)
            mi.call("HYPRE_BoomerAMGSetNumSweeps", amg.h, 2)
            x.fill(0.0)
        assert gm.solve(A, b, x) == 0
        runs.append((gm.num_iterations, np.asarray(gm.residual_history()).copy(), x.get().copy()))
    assert runs[0][0] == runs[1][0]
    assert np.allclose(runs[0][1], runs[1][1], rtol=1e-9, atol=0.0) and np.allclose(runs[0][2], runs[1][2], rtol=0, atol=1e-10)


@pytest.mark.parametrize("n,stencil", [(24, 7)])
def test_default_on_features_against_their_switches(n, stencil):
    """features that are on by default and change the path of every solve, each against its own switch, in a
    process of its own (the switches are read once): the device arena (MI_HYPRE_POOL 2) against the block cache (1) and
    plain hipMalloc (0), skipped zero-fills, the polled Hessenberg column -- all bit for bit the same solve -- and the
    collapsed dense tail, which is the same operator in another summation order (same iteration count, history and
    solution to rounding)."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(**env):
        e = dict(os.environ, **{k: str(v) for k, v in env.items()})
        p = subprocess.run([sys.executable, os.path.join(root, "tests", "env_worker.py"), str(n), str(stencil)], env=e,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-3000:]
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
        return json.loads(line[len("RESULT "):])

    ref = run()
    assert ref["levels"] >= 4 and ref["arena_mapped"] > 0
    for env in ({"MI_HYPRE_POOL": 0}, {"MI_HYPRE_POOL": 1}, {"MI_HYPRE_SKIP_ZERO_FILL": 0}, {"MI_HYPRE_GMRES_POLL": 0},
                {"MI_HYPRE_ARENA_AHEAD": 0}):
        r = run(**env)
        assert r["iters"] == ref["iters"] and r["hist"] == ref["hist"] and r["x"] == ref["x"], env
        if "MI_HYPRE_POOL" in env:
            assert r["arena_mapped"] == 0, env
    # no tail at all
    r = run(MI_HYPRE_DENSE_TAIL_ROWS=0)
    assert r["iters"] == ref["iters"]
    h0 = np.array([float.fromhex(h) for h in ref["hist"]])
    h1 = np.array([float.fromhex(h) for h in r["hist"]])
    assert np.allclose(h0, h1, rtol=1e-8, atol=0.0)
    x0 = np.frombuffer(bytes.fromhex(ref["x"]), dtype=np.float64)
    x1 = np.frombuffer(bytes.fromhex(r["x"]), dtype=np.float64)
    assert np.abs(x0 - x1).max() < 1e-10



@pytest.mark.parametrize("n,stencil", [(40, 7), (24, 27)])
def test_nothing_reads_memory_it_has_not_written(n, stencil):
    """The device arena hands out driver-cleared memory the first time a chunk is used and the last owner's data ever
    after, so code that relies on zeros it never wrote passes a short test and fails in a long run.  With
    MI_HYPRE_POISON_ALLOC=1 every block comes full of 0xFF bytes (NaN / -1): the same setup (device kernels on every level
    above 500 rows) and the same solve, bit for bit, as without."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(**env):
        e = dict(os.environ, MI_HYPRE_DEVICE_SETUP_MIN_ROWS="500", **{k: str(v) for k, v in env.items()})
        p = subprocess.run([sys.executable, os.path.join(root, "tests", "env_worker.py"), str(n), str(stencil)], env=e,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        assert p.returncode == 0, p.stdout[-3000:]
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
        return json.loads(line[len("RESULT "):])

    ref = run()
    r = run(MI_HYPRE_POISON_ALLOC=1)
    assert r["iters"] == ref["iters"] and r["levels"] == ref["levels"]
    assert r["hist"] == ref["hist"] and r["x"] == ref["x"]
