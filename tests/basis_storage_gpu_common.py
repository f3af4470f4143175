"""What tests/test_gpu_basis_storage.py and its child process (tests/basis_storage_worker.py) share: the solves of the
"mode 1 equals mode 2" contract and how a solve runs under a basis storage mode."""
import contextlib
import hashlib

import numpy as np

from tests.systems import convection_diffusion_3d, three_component_rhs

# (id, grid, solver, kdim, cgs, tol, BoomerAMG, max_iter): the 7-point Laplacian at 14^3 with b = A 1; "cd12x3": the
# three-component convection-diffusion multivector at 12^3
SOLVES = [
    ("gmres20_plain", "lap14", "gmres", 20, 0, 1e-8, False, 100),   # blocks of 8 and 16, restarts
    ("gmres5_amg", "lap14", "gmres", 5, 0, 1e-12, True, 60),
    ("gmres40_amg", "lap14", "gmres", 40, 0, 1e-12, True, 80),      # the cycle that cannot reach 1e-12
    ("cogmres1_amg", "lap14", "cogmres", 10, 1, 1e-10, True, 60),
    ("cogmres2_plain", "lap14", "cogmres", 20, 2, 1e-8, False, 100),
    ("fgmres_amg", "lap14", "fgmres", 5, 0, 1e-10, True, 60),
    ("gmres12_three_components", "cd12x3", "gmres", 12, 0, 1e-9, True, 60),
]
AMG_SOLVES = [s[0] for s in SOLVES if s[6]]


def by_id(sid):
    return next(s for s in SOLVES if s[0] == sid)


@contextlib.contextmanager
def basis_storage(mi, mode):
    before = mi.get_basis_storage()
    mi.set_basis_storage(mode)
    try:
        yield
    finally:
        mi.set_basis_storage(before)


def make_solver(mi, spec, amg=True):
    _, _, solver, kdim, cgs, tol, with_amg, max_iter = spec
    kw = dict(tolerance=tol, max_iterations=max_iter, kspace=kdim, print_level=0)
    s = mi.GMRES(**kw) if solver == "gmres" else (mi.FlexGMRES(**kw) if solver == "fgmres" else mi.COGMRES(cgs=cgs, **kw))
    if with_amg and amg:
        s.set_precond(mi.BoomerAMG(print_level=0))
    return s


class Systems:
    """the two systems on the device, built once"""

    def __init__(self, mi):
        self.mi, self._sys = mi, {}

    def get(self, grid):
        mi = self.mi
        if grid not in self._sys:
            if grid == "lap14":
                A, _, _, rhs = mi.build_laplace_system(14, 14, 14, 7)
                self._sys[grid] = (A, rhs[None, :])
            else:
                M = convection_diffusion_3d(12)
                self._sys[grid] = (mi.matrix_from_scipy(M), three_component_rhs(M)[0])
        return self._sys[grid]

    def run(self, spec, mode, solver=None):
        """one solve from a zero guess under a storage mode: dict(code, iters, hist, x, rel)"""
        mi = self.mi
        A, B = self.get(spec[1])
        nc, n = B.shape
        b = mi.IJVector(0, n - 1, B[0]) if nc == 1 else mi.IJVector(0, n - 1, B, ncomp=nc)
        x = mi.IJVector(0, n - 1, np.zeros(n)) if nc == 1 else mi.IJVector(0, n - 1, np.zeros((nc, n)), ncomp=nc)
        s = solver if solver is not None else make_solver(mi, spec)
        with basis_storage(mi, mode):
            s.setup(A, b, x)
            code = s.solve(A, b, x)
        xs = x.get_all().ravel() if nc > 1 else x.get()
        return dict(code=code, iters=s.num_iterations, hist=s.residual_history(), x=xs, rel=s.final_rel_res)


def digest(r):
    h = hashlib.sha256()
    h.update(np.int64(r["iters"]).tobytes())
    h.update(np.ascontiguousarray(r["hist"], dtype=np.float64).tobytes())
    h.update(np.ascontiguousarray(r["x"], dtype=np.float64).tobytes())
    h.update(np.float64(r["rel"]).tobytes())
    return h.hexdigest()
