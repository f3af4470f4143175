"""What tests/test_gpu_krylov_paths.py and its child processes (tests/krylov_worker.py) share: running a case of
tests/krylov_cases.py through the library, and the checks of the Krylov loops' vector kernels through the
HYPRE_MI_VectorKernelOp hook."""
import numpy as np

from tests import krylov_cases as kc

LD = np.longdouble
VEC_N = (1, 2, 3, 511, 512, 513, 1025, 4099)
VEC_M = (1, 7, 8, 9, 16, 17, 20)


def make_solver(mi, solver, case):
    kw = dict(tolerance=case["tol"], max_iterations=case["max_iter"], print_level=0)
    if case["atol"]:
        kw["absolute_tol"] = case["atol"]
    if case["min_iter"]:
        kw["min_iterations"] = case["min_iter"]
    if solver == "pcg":
        return mi.PCG(two_norm=case["two_norm"], **kw)
    if solver == "bicgstab":
        return mi.BiCGSTAB(**kw)
    kw["kspace"] = case["kdim"]
    if solver == "gmres":
        return mi.GMRES(**kw)
    if solver == "fgmres":
        return mi.FlexGMRES(**kw)
    return mi.COGMRES(cgs=int(solver[-1]), **kw)


def vectors(mi, b, x0):
    b, x0 = np.atleast_2d(b), np.atleast_2d(x0)
    nc, n = b.shape
    if nc == 1:
        return mi.IJVector(0, n - 1, b[0]), mi.IJVector(0, n - 1, x0[0])
    return mi.IJVector(0, n - 1, b, ncomp=nc), mi.IJVector(0, n - 1, x0, ncomp=nc)


def solve(mi, s, A, b, x0, A_setup=None, setup=True):
    """Setup on A_setup (default A), Solve on A; the answer as dict(code, iters, hist, x, rel)."""
    bv, xv = vectors(mi, b, x0)
    if setup:
        s.setup(A_setup if A_setup is not None else A, bv, xv)
    code = s.solve(A, bv, xv, allow_generic=True)
    x = xv.get_all().ravel() if xv.ncomp > 1 else xv.get()
    return dict(code=code, iters=s.num_iterations, hist=s.residual_history(), x=x, rel=s.final_rel_res)


def run_case(mi, solver, case, A, amg=None, A_solve=None):
    """A fresh solver object on a case; A: the IJ matrix of the case's operator (Setup, and Solve unless A_solve)."""
    _, b, x0 = kc.system(case)
    s = make_solver(mi, solver, case)
    if amg is not None:
        s.set_precond(amg)
    return solve(mi, s, A_solve if A_solve is not None else A, b, x0, A_setup=A)


def to_json(r):
    return dict(code=r["code"], iters=r["iters"], hist=[float(h).hex() for h in r["hist"]], x=r["x"].tobytes().hex(),
                rel=float(r["rel"]).hex())


def from_json(d):
    return dict(code=d["code"], iters=d["iters"], hist=np.array([float.fromhex(h) for h in d["hist"]]),
                x=np.frombuffer(bytes.fromhex(d["x"]), dtype=np.float64), rel=float.fromhex(d["rel"]))


def same_bits(a, b):
    return (a["code"] == b["code"] and a["iters"] == b["iters"] and a["hist"].tobytes() == b["hist"].tobytes()
            and a["x"].tobytes() == b["x"].tobytes() and np.float64(a["rel"]).tobytes() == np.float64(b["rel"]).tobytes())


def check_against_reference(got, ref, solver, b, x0):
    """iteration count, return code, history within rtol 1e-7 + 1e-13 norms[0], x within 1e-9 max|x_ref|, the final
    relative residual against the restatement's and against the last history entry; no NaN where none belongs."""
    assert got["code"] == ref["code"], (got["code"], ref["code"])
    assert got["iters"] == ref["iters"], (got["iters"], ref["iters"])
    if ref["code"] == 1:  # a NaN in b: nothing happened to x
        assert got["x"].tobytes() == np.ravel(x0).tobytes()
        return
    rn, h = ref["norms"], got["hist"]
    assert len(h) == len(rn), (len(h), len(rn))
    assert not np.isnan(h).any() and not np.isnan(got["x"]).any()
    n0 = rn[0] if len(rn) else 0.0
    if len(rn):
        err = np.abs(h - rn)
        assert np.all(err <= 1e-7 * np.abs(rn) + 1e-13 * n0), (err / (1e-7 * np.abs(rn) + 1e-13 * n0)).max()
    xerr = np.abs(got["x"] - ref["x"]).max()
    assert xerr <= 1e-9 * np.abs(ref["x"]).max(), (xerr, np.abs(ref["x"]).max())
    # the final relative residual is the last estimate (max_iter, PCG) or the true residual of the same iterate, which
    # differs from the estimate by rounding errors of the size the history bound already allows
    # (relative to ||b||, except with b = 0 and in PCG, whose history is relative already)
    bn = np.linalg.norm(np.ravel(b))
    den = 1.0 if (bn == 0.0 or solver == "pcg") else bn
    assert abs(got["rel"] - ref["rel_res"]) <= 1e-7 * ref["rel_res"] + 1e-13 * n0 / den
    if len(h):
        assert abs(got["rel"] * den - h[-1]) <= 1e-7 * h[-1] + 1e-13 * n0


# ------------------------------------------------------------------ vector kernels
def _vec(mi, v):
    return mi.IJVector(0, len(v) - 1, v)


def _dot(mi, x, y):
    prod = mi.c_dbl()
    mi.call("HYPRE_ParVectorInnerProd", x.par, y.par, mi.C.byref(prod))
    return prod.value


def check_vector_kernels(mi, n, ms=VEC_M):
    """mass_dot, mass_axpy, lin_comb (init on and off), axpy_dot (xd given and null) and scale_inv_sqrt_post at one
    vector length: values against extended-precision sums within 1e-13 * sum|terms| (the rule of test_blas1), and the
    claims of the kernels' comments bit for bit -- every block inner product equals the separate inner product, the
    block update equals axpys in ascending j, the linear combination equals the copy / scale / axpy chain, the fused
    update-and-product equals axpy followed by the inner product."""
    rng = np.random.default_rng(1000 + n)
    mmax = max(ms)
    V = rng.standard_normal((mmax, n))
    wv, xdv = rng.standard_normal(n), rng.standard_normal(n)
    Vd = [_vec(mi, v) for v in V]
    w0, xd = _vec(mi, wv), _vec(mi, xdv)
    VL, wL = V.astype(LD), wv.astype(LD)
    for m in ms:
        vecs = Vd[:m]
        coef = rng.standard_normal(m)
        # --- block inner products
        got = mi.vector_kernel_op(mi.VEC_MASS_DOT, vecs, None, w0)
        for j in range(m):
            terms = VL[j] * wL
            assert abs(got[j] - float(terms.sum())) <= 1e-13 * float(np.abs(terms).sum()) + 1e-300, ("mass_dot", n, m, j)
            assert got[j] == _dot(mi, vecs[j], w0), ("mass_dot bits", n, m, j)
        # --- block update, scale -1 as the Gram-Schmidt pass uses it and a scale that is no power of two
        for scale in (-1.0, 0.3):
            w1, w2 = _vec(mi, wv), _vec(mi, wv)
            mi.vector_kernel_op(mi.VEC_MASS_AXPY, vecs, coef, w1, scale=scale)
            for j in range(m):
                mi.call("HYPRE_ParVectorAxpy", scale * coef[j], vecs[j].par, w2.par)
            terms = (LD(scale) * coef.astype(LD))[:, None] * VL[:m]
            bound = 1e-13 * (np.abs(wL) + np.abs(terms).sum(axis=0)).astype(float)
            assert np.all(np.abs(w1.get() - (wL + terms.sum(axis=0)).astype(float)) <= bound), ("mass_axpy", n, m)
            assert w1.get().tobytes() == w2.get().tobytes(), ("mass_axpy bits", n, m, scale)
        # --- linear combination
        for init in (True, False):
            w1, w2 = _vec(mi, wv), _vec(mi, wv)
            mi.vector_kernel_op(mi.VEC_LIN_COMB, vecs, coef, w1, init=init)
            if init:
                mi.call("HYPRE_ParVectorCopy", vecs[0].par, w2.par)
                mi.call("HYPRE_ParVectorScale", float(coef[0]), w2.par)
            for j in range(1 if init else 0, m):
                mi.call("HYPRE_ParVectorAxpy", float(coef[j]), vecs[j].par, w2.par)
            terms = coef.astype(LD)[:, None] * VL[:m]
            base = np.zeros(n, dtype=LD) if init else wL
            bound = 1e-13 * (np.abs(base) + np.abs(terms).sum(axis=0)).astype(float)
            assert np.all(np.abs(w1.get() - (base + terms.sum(axis=0)).astype(float)) <= bound), ("lin_comb", n, m, init)
            assert w1.get().tobytes() == w2.get().tobytes(), ("lin_comb bits", n, m, init)
    # --- fused update and inner product (one vector), the product with another vector and with itself
    for given in (True, False):
        for scale, c in ((-1.0, 0.7310585786300049), (0.3, -2.5)):
            w1, w2 = _vec(mi, wv), _vec(mi, wv)
            got = mi.vector_kernel_op(mi.VEC_AXPY_DOT, Vd[:1], [c], w1, scale=scale, xd=xd if given else None)
            mi.call("HYPRE_ParVectorAxpy", scale * c, Vd[0].par, w2.par)
            want = _dot(mi, xd if given else w2, w2)
            yL = wL + LD(scale) * LD(c) * VL[0]
            terms = (xdv.astype(LD) if given else yL) * yL
            assert abs(got - float(terms.sum())) <= 1e-13 * float(np.abs(terms).sum()) + 1e-300, ("axpy_dot", n, given)
            assert w1.get().tobytes() == w2.get().tobytes() and got == want, ("axpy_dot bits", n, given)
    # --- the scaling kernel that posts the Hessenberg column: slots and flag arrive, the vector is scaled, and a
    #     norm of exactly 0 (lucky breakdown) leaves the vector alone but still posts
    for count in (1, 9, 21, 255):
        slots = rng.standard_normal(count)
        slots[0] = float(wv @ wv)
        w1 = _vec(mi, wv)
        posted, flag, seq = mi.vector_kernel_op(mi.VEC_SCALE_POST, [], slots, w1)
        assert posted.tobytes() == slots.tobytes() and flag == seq, ("scale_post", n, count)
        assert np.all(np.abs(w1.get() - wv / np.sqrt(slots[0])) <= 4e-16 * np.abs(wv / np.sqrt(slots[0]))), ("scale_post", n)
        before = w1.get()
        slots[0] = 0.0
        posted, flag, seq = mi.vector_kernel_op(mi.VEC_SCALE_POST, [], slots, w1)
        assert posted.tobytes() == slots.tobytes() and flag == seq, ("scale_post, norm 0", n, count)
        assert w1.get().tobytes() == before.tobytes(), ("scale_post, norm 0", n)
