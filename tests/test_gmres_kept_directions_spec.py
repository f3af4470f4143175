"""CPU: the two solution updates of GMRES behind a linear preconditioner on the restatement (tests/krylov_ref.gmres):
x += M^-1 sum_j y_j p_j (gmres.c) and x += sum_j y_j z_j with the kept z_j = M^-1 p_j.  With M^-1 a fixed matrix they
are the same vector; the restatement works in extended precision, so on the cases of tests/kept_directions_cases.py the
two must agree far inside the bound the device paths are held to (1e-9 max|x|) -- 1e-13 max|x| is asked here -- with
the same iterations, code and history, and every case must be clear of a coin-flip at its tolerance (no estimate in
(0.9, 1.1) eps), since only then do the device paths count the same iterations.  M is the CPU oracle's default AMG
cycle, tabulated as a dense matrix.  No GPU."""
import numpy as np
import pytest

from tests import kept_directions_cases as kd
from tests import krylov_cases as kc
from tests import krylov_ref as kr

_TAB = {}


def tabulated_cycle(oc, op):
    if op not in _TAB:
        A = kd.operator(op)
        amg = oc.Amg(oc.Csr.from_scipy(A), oc.default_params())
        n = A.shape[0]
        B = np.empty((n, n))
        for j in range(n):
            e = np.zeros(n)
            e[j] = 1.0
            B[:, j] = amg.cycle(e)
        _TAB[op] = B
    return _TAB[op]


def test_exported_and_declared(mi_lib):
    lib = mi_lib.lib()
    assert hasattr(lib, "HYPRE_MI_SetGmresKeepDirections") and hasattr(lib, "HYPRE_MI_TestGmresDirectionAllocFailsAt")


@pytest.mark.parametrize("sc", kd.ALL, ids=kc.case_id)
def test_both_updates_agree_on_the_restatement(oc, sc):
    solver, case = sc
    A, b, x0 = kd.system(case)
    M = kr.dense_precond(tabulated_cycle(oc, case["op"]))
    recomputed = kc.reference("gmres", case, A, b, x0, M)
    kept = kc.reference("fgmres", case, A, b, x0, M)
    assert kept["iters"] == recomputed["iters"] and kept["code"] == recomputed["code"]
    assert recomputed["code"] == (256 if case["max_iter"] < 200 else 0)
    assert recomputed["iters"] > (case["kdim"] if case["kdim"] < 20 else 3)  # k_dim 3: more than one restart cycle
    assert recomputed["iters"] <= 20 or case["kdim"] < 20  # k_dim 20: one restart cycle
    scale = float(np.abs(recomputed["x"]).max())
    assert np.abs(kept["x"] - recomputed["x"]).max() <= 1e-13 * scale
    n0 = recomputed["norms"][0]
    assert np.all(np.abs(kept["norms"] - recomputed["norms"]) <= 1e-8 * np.abs(recomputed["norms"]) + 1e-13 * n0)
    # no tested estimate near the threshold: the last one at most 0.9 eps when the solve converged, all others >= 1.1 eps
    for ref in (kept, recomputed):
        t, eps = np.asarray(ref["tested"], dtype=float), float(ref["eps"])
        assert not np.any((t > 0.9 * eps) & (t < 1.1 * eps)), (t / eps)
