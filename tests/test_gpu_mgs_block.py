"""The blocked modified Gram-Schmidt of single-rank GMRES on the device: one pass of k::mgs_block_pass through the
HYPRE_MI_VectorKernelOp hook against the numpy restatement of tests/test_mgs_block_spec.py, and whole solves against
the CPU oracle's chain MGS (same iteration count, history and final residual within the bars of test_gpu_amg.py)."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.systems import convection_diffusion_3d, three_component_rhs
from tests.test_mgs_block_spec import B, LD, forward_subst

pytestmark = pytest.mark.gpu

# the tail element, one workgroup, just over one grid-stride of the capped grid (768 workgroups x 512), 2^20 + 1
SIZES = (1, 2, 3, 511, 513, 393216 + 3, (1 << 20) + 1)
COUNTS = (0, 1, 7, 8)
ALL_PASSES = [(mp, mn, False) for mp in COUNTS for mn in COUNTS if mp + mn > 0] + [(mp, 0, True) for mp in COUNTS if mp]
# at the two long sizes (the reference sums in extended precision dominate the time): full and partial blocks, no
# block to subtract, both kinds of last pass
FEW_PASSES = [(8, 8, False), (7, 1, False), (0, 8, False), (8, 0, True), (1, 0, True)]


def _vec(mi, v):
    return mi.IJVector(0, len(v) - 1, v)


def _inputs(rng):
    """raw inner products and raw Gram rows with g_jk up to 0.3 in size; row 5 has norm^2 = 0 beside non-zero
    products (its g are 0), row 0's entries are never read"""
    c = rng.standard_normal(B)
    s = rng.uniform(0.01, 100.0, B)
    gram = np.zeros((B, B + 1))
    gram[:, :B] = rng.uniform(-0.3, 0.3, (B, B)) * s[:, None]
    gram[:, B] = s * s
    gram[5, B] = 0.0
    gram[0, :] = np.nan
    return c, gram


def _check_pass(mi, n, Pd, P, Qd, Q, wv, mp, mn, last, c, gram, twice):
    w1 = _vec(mi, wv)
    sums, h, ncopy = mi.mgs_block_pass(Pd[:mp], Qd[:mn], last, c, gram, w1)
    got_w = w1.get()
    if twice:
        w2 = _vec(mi, wv)
        sums2, h2, ncopy2 = mi.mgs_block_pass(Pd[:mp], Qd[:mn], last, c, gram, w2)
        assert sums.tobytes() == sums2.tobytes() and h.tobytes() == h2.tobytes() and ncopy == ncopy2
        assert got_w.tobytes() == w2.get().tobytes()
    tag = (n, mp, mn, last)
    h_ref, g = forward_subst(c, gram, mp)
    amp = float(np.prod(1.0 + np.abs(g)))
    tol_h = np.array([1e-13 * float(abs(LD(c[j])) + (np.abs(h_ref[:j]) * np.abs(g[j, :j])).sum()) * amp if j < mp else 0.0
                      for j in range(B)])
    assert np.all(np.abs(h.astype(LD) - h_ref).astype(float) <= tol_h), ("h", tag)
    assert np.all(h[mp:] == 0.0)
    wL = wv.astype(LD)
    w_ref, absw = wL.copy(), np.abs(wL)
    tol_w = np.zeros(n)
    for j in range(mp):
        w_ref = w_ref - h_ref[j] * P[j]
        absw = absw + np.abs(h_ref[j]) * np.abs(P[j])
        tol_w += tol_h[j] * np.abs(P[j]).astype(float)
    tol_w += 1e-13 * absw.astype(float)
    ew = np.abs(got_w.astype(LD) - w_ref).astype(float)
    assert np.all(ew <= tol_w), ("w", tag, float((ew / tol_w).max()))
    if mp == 0:
        assert got_w.tobytes() == wv.tobytes()
    vecs, cnt = (P, mp) if last else (Q, mn)
    for j in range(cnt):
        terms = vecs[j] * w_ref
        tol = 1e-13 * float(np.abs(terms).sum()) + float((np.abs(vecs[j]).astype(float) * tol_w).sum())
        assert abs(sums[j] - float(terms.sum())) <= tol, ("sum", tag, j, abs(sums[j] - float(terms.sum())) / tol)
    assert np.all(sums[cnt:B] == 0.0)
    if last:
        t = float((w_ref * w_ref).sum())
        tol = 1e-13 * t + 2.0 * float((np.abs(w_ref).astype(float) * tol_w).sum())
        assert abs(sums[B] - t) <= tol, ("norm", tag)
        assert ncopy == sums[B]
    else:
        assert sums[B] == 0.0 and ncopy == 0.0


@pytest.mark.parametrize("n", SIZES)
def test_one_pass_against_the_restatement(mi, n):
    rng = np.random.default_rng(500 + n % 1000)
    Pf, Qf = rng.standard_normal((B, n)), rng.standard_normal((B, n))
    Pd, Qd = [_vec(mi, v) for v in Pf], [_vec(mi, v) for v in Qf]
    P, Q = Pf.astype(LD), Qf.astype(LD)
    wv = rng.standard_normal(n)
    c, gram = _inputs(rng)
    long = n > 100000
    for k, (mp, mn, last) in enumerate(FEW_PASSES if long else ALL_PASSES):
        _check_pass(mi, n, Pd, P, Qd, Q, wv, mp, mn, last, c, gram, twice=(not long) or k == 0)


# ------------------------------------------------------------------ whole solves
def _chunk(mi):
    c = mi.c_int()
    mi.call("HYPRE_MI_GetGSChunk", mi.C.byref(c))
    return c.value


def _compare(gm, info, min_iters):
    print(f"iterations {gm.num_iterations} (oracle {info['iters']}), final rel res {gm.final_rel_res:.6e} "
          f"(oracle {info['rel_res']:.6e})")
    assert gm.num_iterations == info["iters"] and gm.num_iterations >= min_iters
    hist, ref = gm.residual_history(), info["norms"]
    assert len(hist) == len(ref)
    err = np.abs(hist - ref) / (1e-8 * np.abs(ref) + 1e-14 * ref[0])
    print(f"history: largest error / bound {err.max():.3e}")
    assert np.allclose(hist, ref, rtol=1e-8, atol=1e-14 * ref[0])
    assert abs(gm.final_rel_res - info["rel_res"]) <= 1e-10


def test_solver_without_preconditioner_crosses_blocks_and_restarts(mi, oc):
    """GMRES(20): every cycle runs over the block boundaries at 8 and 16 and ends in the partial block 16 .. 19"""
    n = 14
    A, b, x, rhs = mi.build_laplace_system(n, n, n, 7)
    gm = mi.GMRES(tolerance=1e-8, max_iterations=100, kspace=20, print_level=0)
    gm.setup(A, b, x)
    assert gm.solve(A, b, x) == 0
    Ao, bo = oc.Csr.laplace(n, n, n, 7)
    xo, info = oc.gmres(Ao, bo, kdim=20, tol=1e-8, maxit=100, amg=None)
    _compare(gm, info, 21)
    assert np.abs(x.get() - xo).max() <= 1e-9 * np.abs(xo).max()


@pytest.mark.parametrize("kdim", [5, 40])
def test_solver_behind_amg(mi, oc, kdim):
    """kdim 5: restarts inside the first block; kdim 40: one cycle across the boundary at 8"""
    n = 14
    A, b, x, rhs = mi.build_laplace_system(n, n, n, 7)
    amg = mi.BoomerAMG(print_level=0)
    gm = mi.GMRES(tolerance=1e-12, max_iterations=60, kspace=kdim, print_level=0)
    gm.set_precond(amg)
    gm.setup(A, b, x)
    assert gm.solve(A, b, x) == 0
    Ao, bo = oc.Csr.laplace(n, n, n, 7)
    oamg = oc.Amg(Ao, oc.default_params(gs_chunk=_chunk(mi)))
    xo, info = oc.gmres(Ao, bo, kdim=kdim, tol=1e-12, maxit=60, amg=oamg)
    _compare(gm, info, 9)
    assert np.abs(x.get() - xo).max() <= 1e-9 * np.abs(xo).max()


def test_solver_on_a_three_component_multivector(mi, oc):
    """one Krylov space over three components (flat vectors of length 3 n), GMRES(12)"""
    n = 12
    M = convection_diffusion_3d(n)
    Bm, X = three_component_rhs(M)
    N = n ** 3
    A = mi.matrix_from_scipy(M)
    b = mi.IJVector(0, N - 1, Bm, ncomp=3)
    x = mi.IJVector(0, N - 1, np.zeros((3, N)), ncomp=3)
    amg = mi.BoomerAMG(print_level=0)
    gm = mi.GMRES(tolerance=1e-9, max_iterations=60, kspace=12, print_level=0)
    gm.set_precond(amg)
    gm.setup(A, b, x)
    assert gm.solve(A, b, x) == 0
    oamg = oc.Amg(oc.Csr.from_scipy(M), oc.default_params(gs_chunk=_chunk(mi)))
    blk = oc.Csr.from_scipy(sp.kron(sp.eye(3), M).tocsr())
    xo, info = oc.gmres(blk, Bm.ravel(), kdim=12, tol=1e-9, maxit=60, amg=oamg, ncomp=3)
    _compare(gm, info, 9)
    assert np.abs(x.get_all().ravel() - xo).max() <= 1e-9 * np.abs(xo).max()
