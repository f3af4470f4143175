"""C-row hand-over: the C pass that ends a cycle stores (A z)_i for the level-0 C rows whose only
C column is their diagonal, and the Krylov mat-vec w = A z that follows runs on the other tiles alone.

  (a) Laplace 12^3 7-pt (a chunk straddles nc), (b) Laplace 16^3 27-pt, (c) a 16^3 7-pt operator whose z coupling is
      0.5 in the upper half of its planes (weak there: C points couple, so level 0 has handed-over AND listed C tiles):
      after a cycle in mode 2 the reduced mat-vec equals the full one and scipy's A z on every row, 1e-12 max|w|;
      the census' flagged rows are the C rows with an off-diagonal C column of level_csr / level_cf;
  (d) full solves in modes 0 / 1 / 2: same iterations, histories to rtol 1e-9, x to 1e-12, one reduced mat-vec per
      iteration in mode 2 and none in mode 0 (the initial and final residuals stay full);
  (e) relax type 16, relax_order 0, no up sweep, a 3-component multivector: the flag stays down.
Tolerances as in test_gpu_amg.py::test_zero_guess_sub_operator: the paths differ in summation order only.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.handover_cases import half_anisotropic

pytestmark = pytest.mark.gpu

_SYS = {}


def system(mi, case, ncomp=1):
    """(A, b as an array, n) of a case, the matrix once per module"""
    if case not in _SYS:
        if case == "aniso":
            M = half_anisotropic()
            N = M.shape[0]
            A = mi.IJMatrix(0, N - 1)
            coo = M.tocoo()
            A.set_values_coo(coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data)
            A.assemble()
            bv = M @ np.ones(N)
        else:
            n, stencil = case
            A, b, x, rhs = mi.build_laplace_system(n, n, n, stencil)
            bv = b.get()
        _SYS[case] = (A, bv)
    A, bv = _SYS[case]
    return A, bv, len(bv)


@pytest.fixture
def mode(mi):
    yield lambda m: mi.set_c_row_handover(m)
    mi.set_c_row_handover(1)


def level0(amg):
    ia, ja, a, shape = amg.level_csr(0, 0)
    return sp.csr_matrix((a, ja, ia), shape=shape), np.asarray(amg.level_cf(0))


@pytest.mark.parametrize("case,both_kinds", [((12, 7), False), ((16, 27), False), ("aniso", True)],
                         ids=["laplace12_7pt", "laplace16_27pt", "half_anisotropic16"])
def test_reduced_matvec_after_a_cycle(mi, mode, case, both_kinds):
    mode(2)
    A, bv, n = system(mi, case)
    amg = mi.BoomerAMG(print_level=0)
    amg.setup(A)
    M, cf = level0(amg)
    nc = int((cf == 1).sum())
    assert np.all(cf[:nc] == 1)
    cen = amg.c_row_handover_census(0)
    print(f"{case}: n {n}, nc {nc} (nc % 8 = {nc % 8}), census {cen}")
    # the flagged rows: C rows with an off-diagonal C column
    rows = np.repeat(np.arange(n), np.diff(M.indptr))
    coupled = (rows < nc) & (M.indices < nc) & (M.indices != rows)
    flagged = np.zeros(n, dtype=bool)
    flagged[rows[coupled]] = True
    assert cen["flagged_c_rows"] == int(flagged.sum())
    assert cen["handed"] > 0 and cen["listed"] + cen["handed"] == cen["tiles"]
    assert 0 < cen["w_upto"] <= nc
    if both_kinds:
        assert cen["flagged_c_rows"] > 0
        # a listed tile made of C rows alone: a tile has at most 512 rows, so the tile of a flagged row that far
        # below nc ends among the C rows
        assert flagged[:max(nc - 512, 0)].any()
    else:
        assert cen["flagged_c_rows"] == 0
    f = np.random.default_rng(5).standard_normal(n)
    z, w, w_full, raised = amg.cycle_then_matvec(f)
    assert raised
    bound = 1e-12 * np.abs(w_full).max()
    ref = M @ z
    print(f"  max|w - w_full| {np.abs(w - w_full).max():.3e}, max|w - A z| {np.abs(w - ref).max():.3e}, bound {bound:.3e}")
    assert np.isfinite(w).all()
    assert np.abs(w - w_full).max() <= bound
    assert np.abs(w - ref).max() <= bound
    # mode 0: the same cycle, the full mat-vec
    mode(0)
    z0, w0, w0_full, raised0 = amg.cycle_then_matvec(f)
    assert not raised0 and np.array_equal(z0, z) and np.array_equal(w0, w0_full)


def solve(mi, case, m, ncomp=1, **amg_kw):
    A, bv, n = system(mi, case)
    mi.set_c_row_handover(m)
    if ncomp > 1:
        bv = np.stack([bv * (c + 1) for c in range(ncomp)])
    b = mi.IJVector(0, n - 1, bv, ncomp=ncomp)
    x = mi.IJVector(0, n - 1, np.zeros_like(bv), ncomp=ncomp)
    amg = mi.BoomerAMG(print_level=0, **amg_kw)
    gm = mi.GMRES(tolerance=1e-10, max_iterations=100, kspace=50, print_level=0)
    gm.set_precond(amg)
    gm.setup(A, b, x)
    h0 = mi.counter("handover_matvecs")
    assert gm.solve(A, b, x) == 0
    xs = x.get_all().ravel() if ncomp > 1 else x.get()
    return dict(iters=gm.num_iterations, hist=np.asarray(gm.residual_history()), x=xs,
                handed=mi.counter("handover_matvecs") - h0)


@pytest.mark.parametrize("case", [(12, 7), "aniso"], ids=["laplace12_7pt", "half_anisotropic16"])
def test_solves_agree_across_modes(mi, mode, case):
    runs = {m: solve(mi, case, m) for m in (0, 1, 2)}
    for m in (1, 2):
        dx = np.abs(runs[m]["x"] - runs[0]["x"]).max()
        print(f"{case} mode {m}: {runs[m]['iters']} iterations, {runs[m]['handed']} reduced mat-vecs, max|x - x_0| {dx:.3e}")
        assert runs[m]["iters"] == runs[0]["iters"]
        assert np.allclose(runs[m]["hist"], runs[0]["hist"], rtol=1e-9, atol=0.0)
        assert dx <= 1e-12
    assert runs[0]["handed"] == 0
    assert runs[2]["handed"] == runs[2]["iters"]  # one per Arnoldi step; the initial and final residuals are full


@pytest.mark.parametrize("name,ncomp,kw", [
    ("chebyshev", 1, dict(relax_type=16)),
    ("relax_order_0", 1, dict(relax_order=0)),
    ("no_up_sweep", 1, dict(num_down_sweeps=1, num_up_sweeps=0, num_coarse_sweeps=1)),
    ("multivector", 3, dict()),
], ids=lambda v: v if isinstance(v, str) else None)
def test_fallbacks_keep_the_full_matvec(mi, mode, name, ncomp, kw):
    off = solve(mi, (12, 7), 0, ncomp=ncomp, **kw)
    on = solve(mi, (12, 7), 2, ncomp=ncomp, **kw)
    assert on["handed"] == 0 and off["handed"] == 0
    assert on["iters"] == off["iters"]
    assert np.abs(on["x"] - off["x"]).max() <= 1e-12
