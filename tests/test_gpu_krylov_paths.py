"""The Krylov loops of csrc/krylov.cpp beyond the zero-guess, converging solve: every case of tests/krylov_cases.py on
the device against the extended-precision restatement (tests/krylov_ref.py; tests/test_krylov_spec.py pins the
restatement to the CPU oracle and keeps every case clear of its tolerance).

Every solve is checked for its iteration count, its return code (0, 256 = max_iter, 1 = NaN), residual_history()
within rtol 1e-7 + 1e-13 norms[0] (the bound of test_gpu_golden.py and test_gpu_mixed_sign.py), x within
1e-9 max|x_ref| and the final relative residual (krylov_gpu_common.check_against_reference).

Paths named here: a non-zero initial guess in every solver (enter_level_order gathers x, leave_level_order scatters
it, the first residual is b - A x0, PCG's zero-right-hand-side exit overwrites x through the scatter); SetAbsoluteTol,
SetMinIter, PCGSetTwoNorm, COGMRESSetCGS(2) (the second slot block); max_iter inside a restart cycle and at the end of
one; b = 0 (den = ||r0||); r0 = 0 on entry; the lucky breakdown (a new basis vector of norm exactly 0: scale_post_k
returns early); the NaN exit; BiCGSTAB's <r0, A p> = 0 breakdown; restart cycles of 20 vectors (three passes of the
block kernels); the natural-order path when Solve gets another matrix than the preconditioner's or
MI_HYPRE_GMRES_PERMUTED=0; multivectors with odd n; a solver object used again on other vectors and another shape;
the vector kernels on their own, with the bitwise claims of their comments.
Not reached: gamma == 0 -> epsmac in the Givens step needs A v = 0, a singular operator whose solve divides 0 by 0;
BiCGSTAB's rho = 0 and omega = 0 exits (only the first of its three breakdown exits has a case)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import krylov_cases as kc
from tests import krylov_gpu_common as kg
from tests import krylov_ref as kr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_MATS, _TAB = {}, {}


def matrix(mi, op):
    if op not in _MATS:
        _MATS[op] = mi.matrix_from_scipy(kc.operator(op))
    return _MATS[op]


def tabulated_amg(mi, op):
    """The library's own default BoomerAMG cycle on an operator as a dense map: one BoomerAMG.solve with
    max_iterations 1, tolerance 0 per unit vector, once per operator and module."""
    if op not in _TAB:
        A = matrix(mi, op)
        n = kc.operator(op).shape[0]
        amg = mi.BoomerAMG(print_level=0, max_iterations=1, tolerance=0.0)
        amg.setup(A)
        e = mi.IJVector(0, n - 1, np.zeros(n))
        u = mi.IJVector(0, n - 1, np.zeros(n))
        B = np.empty((n, n))
        for j in range(n):
            idx = np.array([max(j - 1, 0), j], dtype=np.int64)
            mi.call("HYPRE_IJVectorSetValues", e.h, 2, idx, np.array([0.0, 1.0]))
            u.fill(0.0)
            amg.solve(A, e, u)
            B[:, j] = u.get()
        _TAB[op] = B
    return _TAB[op]


def run_and_check(mi, solver, case, A_solve=None):
    A, b, x0 = kc.system(case)
    M, amg = None, None
    if case["amg"]:
        M = kr.dense_precond(tabulated_amg(mi, case["op"]))
        amg = mi.BoomerAMG(print_level=0)
    ref = kc.reference(solver, case, A, b, x0, M)
    got = kg.run_case(mi, solver, case, matrix(mi, case["op"]), amg=amg, A_solve=A_solve)
    kg.check_against_reference(got, ref, solver, b, x0)
    return got, ref


@pytest.mark.parametrize("sc", [(s, c) for c in kc.NOPRECOND for s in kc.GMRES_FAMILY], ids=kc.case_id)
def test_no_preconditioner(mi, sc):
    """SetPrecond never called (apply_precond copies), x0 != 0, n = 343: 40 iterations in cycles of 20 vectors (block
    kernels in passes of 8, 8 and 4; COGMRES cgs 2 through the second slot block), max_iter at the end of a cycle
    and inside one (code 256, x from a partial basis), b = 0, an absolute tolerance, min_iter beyond the iteration
    that meets the tolerance, a NaN in b (code 1, x bitwise unchanged)."""
    got, ref = run_and_check(mi, *sc)
    if sc[1]["id"] == "cap17_midcycle":
        assert got["code"] == 256 and got["iters"] == 17


@pytest.mark.parametrize("sc", [(s, c) for c in kc.DEGENERATE for s in kc.ALL_SOLVERS] +
                         [(s, kc.LUCKY) for s in kc.GMRES_FAMILY], ids=kc.case_id)
def test_exact_and_degenerate(mi, sc):
    """2 I (one step), an exact guess (r0 = 0 on entry: no iteration -- PCG, which has no test before its first step,
    leaves the loop inside iteration 1 -- and x bitwise equal to x0), three eigenvalues (three steps), and for the
    GMRES family a right-hand side for which every operation is exact and the new basis vector has norm 0 (lucky
    breakdown).  No NaN in x or in the history."""
    solver, case = sc
    got, ref = run_and_check(mi, solver, case)
    if case["id"] == "exact_guess":
        assert got["iters"] == (1 if solver == "pcg" else 0) and got["code"] == 0
        assert got["x"].tobytes() == kc.system(case)[2].tobytes()
    if case["id"] == "three_eigenvalues":
        assert got["iters"] == 3
    if case["id"] == "lucky_breakdown":
        assert got["iters"] == 1 and got["hist"][1] == 0.0 and got["x"].tobytes() == (kc.system(case)[1] / 2.0).tobytes()


@pytest.mark.parametrize("case", kc.BICGSTAB, ids=lambda c: c["id"])
def test_bicgstab_paths(mi, case):
    """x0 != 0, b = 0, max_iter 3 (code 256), an absolute tolerance, the <r0, A p> = 0 breakdown exit (code 0 after one
    iteration, x untouched), a NaN in b."""
    got, ref = run_and_check(mi, "bicgstab", case)
    if case["id"] == "bicgstab_breakdown":
        assert (got["iters"], got["code"]) == (1, 0) and not got["x"].any()


@pytest.mark.parametrize("case", kc.PCG + kc.PCG_AMG, ids=lambda c: c["id"])
def test_pcg_paths(mi, case):
    """The 7-point Laplacian on 7^3 without and with BoomerAMG: x0 != 0, two_norm 0 and 1, an absolute tolerance,
    b = 0 with x0 != 0 (x exactly 0, no iteration, code 0 -- in level order through the scatter), a NaN in b."""
    got, ref = run_and_check(mi, "pcg", case)
    if case["b"] == "zero":
        assert (got["iters"], got["code"]) == (0, 0) and not got["x"].any() and not np.signbit(got["x"]).any()


@pytest.fixture(scope="module")
def natural_order_child():
    """the BoomerAMG-preconditioned cases in a child process with MI_HYPRE_GMRES_PERMUTED=0"""
    return _child("amg", MI_HYPRE_GMRES_PERMUTED=0)


def _child(mode, **env):
    e = dict(os.environ, **{k: str(v) for k, v in env.items()})
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "krylov_worker.py"), mode],
                       env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return {k: kg.from_json(v) for k, v in json.loads(line[len("RESULT "):]).items()}


@pytest.mark.parametrize("sc", kc.AMG, ids=kc.case_id)
def test_amg_preconditioned_three_ways(mi, natural_order_child, sc):
    """n = 729, x0 != 0, GMRES with k_dim 3 and 50, FlexGMRES with k_dim 3, BiCGSTAB, against the restatement with the
    tabulated cycle: (i) in level order (x0 gathered, x scattered back), (ii) Solve on a second IJ matrix with the
    same entries (amg_in_level_order returns null: natural order), (iii) in a process with
    MI_HYPRE_GMRES_PERMUTED=0.  (ii) and (iii) run the same code on the same numbers: bit for bit."""
    solver, case = sc
    run_and_check(mi, solver, case)
    A2 = mi.matrix_from_scipy(kc.operator(case["op"]))
    got2, ref = run_and_check(mi, solver, case, A_solve=A2)
    got3 = natural_order_child[kc.case_id(sc)]
    _, b, x0 = kc.system(case)
    kg.check_against_reference(got3, ref, solver, b, x0)
    assert kg.same_bits(got2, got3)


@pytest.mark.parametrize("sc", kc.MULTI, ids=kc.case_id)
def test_multicomponent(mi, sc):
    """Three components on n = 343 and 729 (odd: components 1 and 2 start 8-byte-aligned only), another random x0 per
    component: GMRES k_dim 5 without a preconditioner (max_iter 60), GMRES and BiCGSTAB with BoomerAMG, against the
    restatement on kron(I_3, A) with the preconditioner applied per component."""
    run_and_check(mi, *sc)


@pytest.mark.parametrize("precond", [False, True], ids=["plain", "amg"])
def test_solver_object_reuse(mi, precond):
    """One GMRES object: case A, then another b and x0 on the same shape (the basis is kept), then after a Setup on the
    n = 729 system that one (the basis is dropped), then case A again.  Each answer equals a fresh object's bit for
    bit."""
    base = kc.make_case("reuse", "cd7", tol=1e-9 if not precond else 1e-10, amg=precond)
    rng = np.random.default_rng(21)
    A7, A9 = kc.operator("cd7"), kc.operator("cd9")
    sysA = kc.system(base)[1:]
    sysB = (A7 @ rng.standard_normal(343), rng.standard_normal(343))
    sysC = (A9 @ rng.standard_normal(729), rng.standard_normal(729))
    steps = [("cd7", sysA, True), ("cd7", sysB, False), ("cd9", sysC, True), ("cd7", sysA, True)]

    def solver():
        s = kg.make_solver(mi, "gmres", base)
        if precond:
            s.set_precond(mi.BoomerAMG(print_level=0))
        return s

    one = solver()
    for op, (b, x0), setup in steps:
        got = kg.solve(mi, one, matrix(mi, op), b, x0, setup=setup)
        fresh = kg.solve(mi, solver(), matrix(mi, op), b, x0)
        assert got["iters"] > 5
        assert kg.same_bits(got, fresh), (op, got["iters"], fresh["iters"])


@pytest.mark.parametrize("n", kg.VEC_N)
def test_vector_kernels(mi, n):
    """k::mass_dot, k::mass_axpy, k::lin_comb, k::axpy_dot and k::scale_inv_sqrt_post through HYPRE_MI_VectorKernelOp,
    m in {1, 7, 8, 9, 16, 17, 20} vectors (one, two and three passes of 8; coef_dev + j0; lin_comb_k<false> after the
    first pass), init on and off, xd given and null: values within 1e-13 sum|terms| of extended-precision sums, and
    bit for bit what the kernels' comments claim (krylov_gpu_common.check_vector_kernels)."""
    kg.check_vector_kernels(mi, n)


def test_vector_kernels_with_two_workgroups_and_unpolled_gmres():
    """The same vector-kernel checks in a child process with MI_HYPRE_VEC_BLOCKS=2 (n = 4099 takes five grid-stride
    trips; MI_HYPRE_DOT_BLOCKS stays unset so that dot and mass_dot share a grid), which also runs the converging
    unpreconditioned GMRES and COGMRES cgs 2 cases; a second child adds MI_HYPRE_GMRES_POLL=0 (copy and
    synchronise instead of the posted Hessenberg column): bit for bit the polled run."""
    polled = _child("vec", MI_HYPRE_VEC_BLOCKS=2)
    unpolled = _child("solves", MI_HYPRE_VEC_BLOCKS=2, MI_HYPRE_GMRES_POLL=0)
    case = kc.NOPRECOND[0]
    A, b, x0 = kc.system(case)
    for solver in ("gmres", "cogmres2"):
        cid = kc.case_id((solver, case))
        kg.check_against_reference(polled[cid], kc.reference(solver, case, A, b, x0), solver, b, x0)
        assert kg.same_bits(polled[cid], unpolled[cid]), cid
