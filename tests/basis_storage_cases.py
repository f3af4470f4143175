"""Cases shared by tests/test_basis_storage_spec.py (CPU: which of them qualify, and the history bar) and
tests/test_gpu_basis_storage.py (device: basis storage mode 2 against tests/basis_storage_ref.py on the qualifying ones).

A case: an operator (7-point Laplacian `lapN` or the seeded convection-diffusion stand-in `cdN` on an N^3 grid), right-hand
sides b_c = A x_c, a zero initial guess, a solver of the GMRES family and its parameters.  `amg`: preconditioned by one
BoomerAMG cycle with default settings -- on the CPU the oracle's cycle, on the device the library's own, both tabulated
column by column as a dense map.

HISTORY_BAR -- measured, not chosen.  tests/basis_storage_ref.gmres runs every case of CASES -- the cases the device
test runs -- twice: in np.longdouble with two Gram-Schmidt passes, and in float64 with the single modified Gram-Schmidt
pass of the device loop.  Both round the stored basis through float32.  The two histories differ because a last-bit
difference in w can turn the float32 rounding of an element of p_i the other way: an error of 2^-24 relative in that
element, not of 2^-53.  The largest deviation of any history entry, relative to ||r_0||: 7.471e-09 (cd7_cogmres2_gmres20;
the lap9 cases 2.9e-09 to 3.2e-09, the cd7 multivector 4.1e-11).  Times 10, rounded up in the third digit: the bar.
test_basis_storage_spec.test_history_bar_is_the_measured_one measures it again and fails when ten times the
measurement leaves [HISTORY_BAR / 1.05, HISTORY_BAR].

A case qualifies for the comparison of iteration counts when every value its longdouble run compared with eps stays
further from eps than HISTORY_BAR * ||r_0||: a run within the bar then takes the same decisions.  Every case of CASES
qualifies; measured margins: lap9_amg_gmres3_restarts 8.3e-06, lap9_amg_gmres2_three_cycles 8.4e-07, lap9_amg_gmres30
and lap9_amg_fgmres10 8.7e-06, cd7_amg_gmres12_three_components 5.1e-06, cd7_cogmres2_gmres20 5.5e-07.  TURNED_AWAY
holds the case the rule rejects: lap8_gmres5_restarts, 38 iterations that creep past eps (margin 6.1e-08).  It runs on
the CPU only and takes no part in the measurement of the bar."""
import numpy as np
import scipy.sparse as sp

from tests import basis_storage_ref as ref
from tests.systems import convection_diffusion_3d, three_component_rhs

HISTORY_BAR = 7.48e-08


def make_case(cid, op, solver="gmres", kdim=20, tol=1e-6, amg=False, ncomp=1, max_iter=200, cgs=0):
    return dict(id=cid, op=op, solver=solver, kdim=kdim, tol=tol, amg=amg, ncomp=ncomp, max_iter=max_iter, cgs=cgs)


CASES = [
    make_case("lap9_amg_gmres3_restarts", "lap9", kdim=3, tol=1e-5, amg=True),
    make_case("lap9_amg_gmres2_three_cycles", "lap9", kdim=2, tol=1e-6, amg=True),
    make_case("lap9_amg_gmres30", "lap9", kdim=30, tol=1e-5, amg=True),
    make_case("cd7_amg_gmres12_three_components", "cd7", kdim=12, tol=1e-5, amg=True, ncomp=3),
    make_case("lap9_amg_fgmres10", "lap9", solver="fgmres", kdim=10, tol=1e-5, amg=True),
    make_case("cd7_cogmres2_gmres20", "cd7", solver="cogmres", cgs=2, kdim=20, tol=1e-5),
]
# decided on the CPU by the restatement alone (test_basis_storage_spec.test_the_listed_cases_qualify)
QUALIFYING = [c["id"] for c in CASES]
RESTARTING = ("lap9_amg_gmres3_restarts", "lap9_amg_gmres2_three_cycles", "cd7_cogmres2_gmres20")
TURNED_AWAY = [make_case("lap8_gmres5_restarts", "lap8", kdim=5, tol=1e-5)]

_OPS = {}


def by_id(cid):
    return next(c for c in CASES + TURNED_AWAY if c["id"] == cid)


def operator(op):
    """scipy CSR"""
    if op not in _OPS:
        n = int(op[-1])
        if op.startswith("lap"):
            T = sp.diags([-np.ones(n - 1), 2 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1])
            eye = sp.identity(n)
            A = sp.kron(sp.kron(T, eye), eye) + sp.kron(sp.kron(eye, T), eye) + sp.kron(sp.kron(eye, eye), T)
            A = sp.csr_matrix(A)
            A.sort_indices()
        else:
            A = convection_diffusion_3d(n)
        _OPS[op] = A
    return _OPS[op]


def rhs(case):
    """(ncomp, N) right-hand sides, component-major"""
    A = operator(case["op"])
    if case["ncomp"] == 1:
        return (A @ np.ones(A.shape[0]))[None, :]
    assert case["ncomp"] == 3
    return three_component_rhs(A)[0]


def reference(case, B=None, arith="longdouble", rounding=True):
    """the restatement on kron(I_ncomp, A); B: the tabulated preconditioner of one component (None: none)"""
    A = operator(case["op"]).toarray()
    nc = case["ncomp"]
    Ab = np.kron(np.eye(nc), A) if nc > 1 else A
    M = ref.per_component(ref.dense_precond(B, arith), nc) if B is not None else None
    return ref.gmres(Ab, rhs(case).ravel(), M=M, tol=case["tol"], max_iter=case["max_iter"], kdim=case["kdim"],
                     flexible=case["solver"] == "fgmres", rounding=rounding, arith=arith)


def history_deviation(r1, r2):
    """largest difference of two histories relative to ||r_0||; inf when they differ in length"""
    if len(r1["norms"]) != len(r2["norms"]):
        return float("inf")
    return float(np.abs(r1["norms"] - r2["norms"]).max() / r1["norms"][0])


def margin(r):
    """the smallest distance of a tested value from eps, relative to ||r_0||"""
    return float(np.abs(r["tested"] - r["eps"]).min() / r["norms"][0])
