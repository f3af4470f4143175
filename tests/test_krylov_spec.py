"""The extended-precision restatements of the Krylov solvers (tests/krylov_ref.py) against the CPU oracle, scipy and
dense solves, on the case table the device tests use (tests/krylov_cases.py).  No GPU.

For every case:
  (a) the oracle and the restatement make the same number of iterations and end the same way;
  (b) no value the solver compares with its threshold eps lies in (0.9, 1.1) eps -- the estimate that ends a solve is
      at most 0.9 eps, every earlier one (and every one of a solve that max_iter ends) at least 1.1 eps -- so that a
      rounding error of the device loops can never change an iteration count: a failure there is a finding;
  (c) the histories agree within rtol 1e-8 + 1e-13 norms[0] and the solutions within 1e-11 max|x|, a factor 10 / 100
      below the bounds of tests/test_gpu_krylov_paths.py.
A case that misses (b) or (c) gets another input (see the note on tolerances in krylov_cases.py), never a wider bound.

The oracle has no min_iter, no two_norm 1 and no NaN test: those cases are checked against the restatement's own
invariants and against oracle runs that express the same iterate in another way."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

from tests import krylov_cases as kc
from tests import krylov_ref as kr

CASES = kc.all_cases()
_TAB = {}


def tabulated_amg(oc, op):
    """(the oracle's default AMG on an operator, its cycle as a dense matrix: one cycle per unit vector)"""
    if op not in _TAB:
        A = kc.operator(op)
        amg = oc.Amg(oc.Csr.from_scipy(A), oc.default_params())
        n = A.shape[0]
        B = np.empty((n, n))
        for j in range(n):
            e = np.zeros(n)
            e[j] = 1.0
            B[:, j] = amg.cycle(e)
        _TAB[op] = (amg, B)
    return _TAB[op]


def _oracle(oc, solver, case, A, b, x0, amg, **over):
    nc = case["ncomp"]
    Ao = oc.Csr.from_scipy(sp.kron(sp.eye(nc), A).tocsr() if nc > 1 else A)
    kw = dict(x0=np.ravel(x0), tol=case["tol"], atol=case["atol"], maxit=case["max_iter"], amg=amg)
    kw.update(over)
    if nc > 1:
        kw["ncomp"] = nc
    bb = np.ravel(b)
    if solver == "pcg":
        return oc.pcg(Ao, bb, **kw)
    if solver == "bicgstab":
        return oc.bicgstab(Ao, bb, **kw)
    if solver == "gmres":
        return oc.gmres(Ao, bb, kdim=case["kdim"], **kw)
    if solver == "fgmres":
        return oc.fgmres(Ao, bb, kdim=case["kdim"], **kw)
    return oc.cogmres(Ao, bb, kdim=case["kdim"], cgs=int(solver[-1]), **kw)


def _assert_close(ref, norms, x):
    rn = ref["norms"]
    if len(norms) > len(rn):  # the oracle hands out iters + 1 entries; a step left by a breakdown wrote none (NaN)
        assert np.all(np.isnan(norms[len(rn):]))
        norms = norms[:len(rn)]
    assert len(norms) == len(rn)
    if len(rn):
        assert np.all(np.abs(norms - rn) <= 1e-8 * np.abs(rn) + 1e-13 * rn[0]), np.abs(norms - rn).max()
    assert np.abs(x - ref["x"]).max() <= 1e-11 * np.abs(ref["x"]).max()


@pytest.mark.parametrize("sc", CASES, ids=kc.case_id)
def test_restatement_against_oracle(oc, sc):
    solver, case = sc
    A, b, x0 = kc.system(case)
    amg, M = None, None
    if case["amg"]:
        amg, B = tabulated_amg(oc, case["op"])
        M = kr.dense_precond(B)
    ref = kc.reference(solver, case, A, b, x0, M)

    # (b) the stopping margin -- a condition on the case, not a measurement of the code
    eps, tested = ref["eps"], ref["tested"]
    if case["b"] != "nan":
        assert not np.any((tested > 0.9 * eps) & (tested < 1.1 * eps)), (eps, tested / eps)
        if ref["converged"] and ref["iters"]:
            # only the estimate that ends the solve, and the true residual that confirms it, are below eps
            assert tested[-1] <= 0.9 * eps and np.sum(tested <= 0.9 * eps) <= 2
        elif ref["code"] == 256:
            assert np.all(tested >= 1.1 * eps)
    assert ref["code"] == (1 if case["b"] == "nan" else 0 if ref["converged"] or ref["iters"] < case["max_iter"] else 256)

    if case["b"] == "nan":  # gmres.c's IEEE check: no iteration, x untouched
        assert ref["iters"] == 0 and np.array_equal(ref["x"], np.ravel(x0)) and not ref["converged"]
        return
    if case["min_iter"]:
        # met after MIN_ITER_OWN iterations, made to go on for four more: the iterate of a solve that max_iter ends
        # at the same count, which the oracle can express
        own = kc.reference(solver, dict(case, min_iter=0), A, b, x0, M)
        xo, info = _oracle(oc, solver, case, A, b, x0, amg)
        assert own["iters"] == info["iters"] == kc.MIN_ITER_OWN and ref["iters"] == case["min_iter"]
        xo, info = _oracle(oc, solver, case, A, b, x0, amg, tol=0.0, maxit=case["min_iter"])
        _assert_close(ref, info["norms"], xo)
        return
    if case["two_norm"]:
        # without a preconditioner the two measures are the same number; with one, only the measure differs: the
        # iterates are those of the two_norm 0 solve as far as this one goes
        other = kc.reference(solver, dict(case, two_norm=0, tol=0.0, max_iter=ref["iters"]), A, b, x0, M)
        assert np.abs(other["x"] - ref["x"]).max() <= 1e-15 * np.abs(ref["x"]).max()
        Ad = A.toarray()
        r = np.ravel(b) - Ad @ ref["x"]
        assert abs(np.linalg.norm(r) / np.linalg.norm(b) - ref["norms"][-1]) <= 1e-6 * ref["norms"][-1]
        if M is None:
            assert np.array_equal(other["norms"], ref["norms"])
        return

    xo, info = _oracle(oc, solver, case, A, b, x0, amg)
    # (a)
    assert info["iters"] == ref["iters"] and info["converged"] == ref["converged"]
    # (c)
    _assert_close(ref, info["norms"], xo)
    if len(ref["norms"]):
        assert abs(info["rel_res"] - ref["rel_res"]) <= 1e-7 * ref["rel_res"] + 1e-13 * ref["norms"][0]


def test_expected_paths_of_the_table():
    """The table reaches what it is meant to reach: full cycles of 20 vectors, an end of max_iter inside a cycle and at
    the end of one, the exits without an iteration, the exact three-step solves."""
    got = {}
    for s, c in CASES:
        if c["amg"] or c["ncomp"] > 1:
            continue
        A, b, x0 = kc.system(c)
        got[kc.case_id((s, c))] = kc.reference(s, c, A, b, x0)
    for s in kc.GMRES_FAMILY:
        assert got[f"{s}-converge_k20"]["iters"] == 40 and got[f"{s}-converge_k20"]["code"] == 0
        assert (got[f"{s}-restart_k5_cap60"]["iters"], got[f"{s}-restart_k5_cap60"]["code"]) == (60, 256)
        assert (got[f"{s}-cap17_midcycle"]["iters"], got[f"{s}-cap17_midcycle"]["code"]) == (17, 256)
        assert got[f"{s}-atol"]["iters"] == 22 and got[f"{s}-min_iter"]["iters"] == kc.MIN_ITER_OWN + 4
        assert got[f"{s}-lucky_breakdown"]["iters"] == 1 and got[f"{s}-lucky_breakdown"]["norms"][1] == 0.0
    for s in kc.ALL_SOLVERS:
        assert got[f"{s}-two_i"]["iters"] == 1 and got[f"{s}-three_eigenvalues"]["iters"] == 3
        # pcg.c has no test before its first step: an exact guess leaves the loop inside iteration 1 (<A p, p> = 0)
        assert got[f"{s}-exact_guess"]["iters"] == (1 if s == "pcg" else 0)
        assert np.array_equal(got[f"{s}-exact_guess"]["x"], kc.system(kc.DEGENERATE[1])[2])
    assert got["bicgstab-bicgstab_cap3"]["code"] == 256
    br = got["bicgstab-bicgstab_breakdown"]
    assert (br["iters"], br["code"], br["converged"]) == (1, 0, False) and not br["x"].any()
    z = got["pcg-pcg_b_zero"]
    assert (z["iters"], z["code"], z["converged"]) == (0, 0, True) and not z["x"].any()


def test_restatement_against_scipy_and_dense_solves():
    A, b, x0 = kc.system(kc.NOPRECOND[0])
    xd = np.linalg.solve(A.toarray(), b)
    ref = kr.gmres(A.toarray(), b, x0=x0, tol=1e-12, max_iter=400, kdim=400)
    assert ref["converged"] and np.abs(ref["x"] - xd).max() <= 1e-10 * np.abs(xd).max()
    # scipy's restarted GMRES with the same restart length reaches the tolerance in the same number of cycles
    xs, _ = spl.gmres(A, b, x0=x0, rtol=1e-9, restart=20, maxiter=10)
    assert np.abs(kr.gmres(A.toarray(), b, x0=x0, tol=1e-9, kdim=20, max_iter=200)["x"] - xs).max() <= 1e-6 * np.abs(xs).max()
    L, bl, xl = kc.system(kc.PCG[0])
    xd = np.linalg.solve(L.toarray(), bl)
    ref = kr.pcg(L.toarray(), bl, x0=xl, tol=1e-13, max_iter=400)
    assert ref["converged"] and np.abs(ref["x"] - xd).max() <= 1e-11 * np.abs(xd).max()
    # conjugate gradients are conjugate gradients: scipy's iterates after k steps are the restatement's
    k = 10
    xs, _ = spl.cg(L, bl, x0=xl, rtol=0.0, maxiter=k)
    assert np.abs(kr.pcg(L.toarray(), bl, x0=xl, tol=0.0, max_iter=k)["x"] - xs).max() <= 1e-12 * np.abs(xs).max()
    ref = kr.bicgstab(A.toarray(), b, x0=x0, tol=1e-12, max_iter=400)
    assert ref["converged"] and np.abs(ref["x"] - np.linalg.solve(A.toarray(), b)).max() <= 1e-10


def test_least_squares_of_the_restatement():
    """lstsq_residual (Householder QR in extended precision) against numpy's lstsq on random Hessenberg matrices"""
    rng = np.random.default_rng(11)
    for k in (1, 2, 7, 20):
        H = np.triu(rng.standard_normal((k + 1, k)), -1)
        y, res = kr.lstsq_residual(H, 3.0)
        rhs = np.zeros(k + 1)
        rhs[0] = 3.0
        yn = np.linalg.lstsq(H, rhs, rcond=None)[0]
        assert np.allclose(np.asarray(y, dtype=float), yn, rtol=1e-9, atol=1e-12)
        assert abs(float(res) - np.linalg.norm(rhs - H @ yn)) <= 1e-12
