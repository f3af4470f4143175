"""Systems and cases of the kept-directions tests (tests/test_gmres_kept_directions_spec.py on the CPU,
tests/test_gpu_gmres_kept_directions.py and tests/kept_directions_worker.py on the device).

GMRES and COGMRES behind a level-ordered BoomerAMG update x += sum_j y_j z_j from the z_j = M^-1 p_j of the Arnoldi
steps ("kept") where gmres.c computes x += M^-1 sum_j y_j p_j ("recomputed").  tests/krylov_ref.gmres states both:
flexible=True is the first formula, flexible=False the second, everything else (Arnoldi process, restart from the
explicit residual) shared."""
import numpy as np
import scipy.sparse as sp

from tests import krylov_cases as kc


def operator(name):
    """lap12: the 7-point Laplacian on 12^3 = 1728 points; every other name is tests/krylov_cases.operator's
    (lap7: 343 rows, cd7 / cd9: the non-symmetric convection-diffusion operator on 343 / 729 rows)"""
    if name != "lap12":
        return kc.operator(name)
    if name not in kc._OPS:
        T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(12, 12))
        I = sp.identity(12)
        M = (sp.kron(sp.kron(T, I), I) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(I, I), T)).tocsr()
        M.sort_indices()
        kc._OPS[name] = M
    return kc._OPS[name]


def system(case, seed=3):
    """(A, b, x0) as tests/krylov_cases.system makes them (b = A times a seeded vector, a random x0), on any operator of
    this module"""
    A = operator(case["op"])
    n, nc = A.shape[0], case.get("ncomp", 1)
    rng = np.random.default_rng(seed)
    xs = rng.standard_normal((nc, n))
    x0 = rng.standard_normal((nc, n))
    b = np.stack([A @ v for v in xs])
    return (A, b[0], x0[0]) if nc == 1 else (A, b, x0)


def _c(id, op, **kw):
    return kc.make_case(id, op, **dict(dict(tol=1e-10, amg=True), **kw))


# (solver, case).  k_dim 20 holds every one of these solves in one restart cycle; k_dim 3 restarts several times
# (updates from full bases, the last one from a partial one; basis and z vectors used again in every cycle);
# max_iter 5 with k_dim 3 ends inside the second restart cycle (code 256).
BASE = [("gmres", _c("lap7", "lap7")), ("gmres", _c("lap12", "lap12")), ("gmres", _c("cd7", "cd7")),
        ("gmres", _c("cd9", "cd9"))]
RESTARTS = [("gmres", _c("cd7_k3", "cd7", kdim=3)), ("gmres", _c("cd9_k3", "cd9", kdim=3))]
CUT_SHORT = [("gmres", _c("cd7_k3_cap5", "cd7", kdim=3, max_iter=5))]
COGMRES = [("cogmres1", _c("cd9_cgs1", "cd9")), ("cogmres2", _c("cd9_cgs2_k3", "cd9", kdim=3))]
# (tol 3e-10: at 1e-10 the ninth estimate of the three-component system is 1.04 eps, a coin-flip -- the spec test's
# condition on the inputs)
MULTI = [("gmres", _c("lap7_3comp", "lap7", ncomp=3, tol=3e-10)),
         ("gmres", _c("lap7_3comp_k3", "lap7", ncomp=3, kdim=3, tol=3e-10))]
ALL = BASE + RESTARTS + CUT_SHORT + COGMRES + MULTI


def updates(iters, kdim):
    """solution updates of a solve without a false convergence: one per restart cycle"""
    return -(-iters // kdim)


def x_bound(x_ref):
    """the project's bound on x (tests/krylov_gpu_common.check_against_reference)"""
    return 1e-9 * float(np.abs(x_ref).max())
