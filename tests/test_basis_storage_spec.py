"""CPU: the specification of the Krylov basis storage modes.  tests/basis_storage_ref.py restates
restarted right-preconditioned GMRES with the basis rounded through float32; here it is pinned to the existing
restatement where the two must agree, shown to have the character the mode was proposed with, and used to measure the
history bar and to pick the cases of tests/test_gpu_basis_storage.py.  Also: the new ABI is exported and refuses what
it must (no device needed).

The five emulation cases: 7-point Laplacian, b = A 1, x0 = 0, M = dense symmetric Gauss-Seidel, fp64 basis against fp32
basis (iterations; false convergences of the fp32 run):
    GMRES(20), 14^3, no preconditioner, tol 1e-8     60 / 60
    GMRES(5),  14^3, tol 1e-12                       48 / 48
    GMRES(12), 12^3, tol 1e-9                        23 / 23
    GMRES(50), 14^3, tol 1e-8                        20 / 21, one false convergence
    GMRES(40), 14^3, tol 1e-12                       27 / 39, one false convergence: the Hessenberg estimate of the first
        cycle goes on falling to eps at iteration 27 while the true residual stands at 2.3e-09 ||r_0||; the second cycle
        does the rest
The counts are those of this restatement with this right-hand side; the emulation the mode was proposed with gave 69 / 69,
42 / 42, 23 / 23, 20 / 21 and 30 / 53 -- the same character case by case, which is what is asserted."""
import numpy as np
import pytest

from tests import basis_storage_cases as bc
from tests import basis_storage_ref as ref
from tests import krylov_ref as kr

_SYS = {}


def _laplace(n):
    if n not in _SYS:
        A = ref.laplace_7pt(n)
        _SYS[n] = (A, A @ np.ones(n ** 3), ref.sgs_matrix(A))
    return _SYS[n]


def _pair(n, kdim, tol, precond):
    A, b, B = _laplace(n)
    M = ref.dense_precond(B) if precond else None
    kw = dict(M=M, tol=tol, kdim=kdim, max_iter=300)
    r64, r32 = ref.gmres(A, b, rounding=False, **kw), ref.gmres(A, b, **kw)
    for r in (r64, r32):  # the returned x confirms the convergence it reports
        assert r["converged"] and r["code"] == 0
        assert np.linalg.norm(b - A @ r["x"]) <= r["eps"] * (1 + 1e-12)
    print(f"GMRES({kdim}) {n}^3 tol {tol}: fp64 basis {r64['iters']}, fp32 basis {r32['iters']} iterations, "
          f"{r32['false_convergences']} false convergence(s)")
    return r64, r32


@pytest.mark.parametrize("n,kdim,tol,precond", [(14, 20, 1e-8, False), (14, 5, 1e-12, True), (12, 12, 1e-9, True)],
                         ids=["gmres20_plain_1e-8", "gmres5_1e-12", "gmres12_12cubed_1e-9"])
def test_free_where_a_cycle_is_asked_for_few_digits(n, kdim, tol, precond):
    """restart cycles that gain at most about 6 digits each: the same iteration count, no false convergence"""
    r64, r32 = _pair(n, kdim, tol, precond)
    assert r32["iters"] == r64["iters"] and r32["false_convergences"] == 0 == r64["false_convergences"]


def test_one_false_convergence_at_eight_digits_in_one_cycle():
    """GMRES(50) to 1e-8: the estimate meets eps one iteration before the true residual does"""
    r64, r32 = _pair(14, 50, 1e-8, True)
    assert r64["false_convergences"] == 0 and r64["iters"] < 50
    assert r32["false_convergences"] == 1 and r32["iters"] == r64["iters"] + 1


def test_a_cycle_gains_about_seven_digits_and_the_restart_recovers():
    """GMRES(40) to 1e-12: the fp64 basis converges inside one cycle; with the fp32 basis the cycle's true residual stays
    above 1e-10 ||r_0|| whatever its estimate says, and only a second cycle, started from b - A x, reaches 1e-12"""
    r64, r32 = _pair(14, 40, 1e-12, True)
    assert r64["iters"] < 40 and r64["false_convergences"] == 0
    assert r32["false_convergences"] >= 1 and r32["iters"] > r64["iters"] + 5
    n0 = r32["norms"][0]
    # `tested` holds the true residual after the first cycle right behind the estimate that claimed convergence
    t = r32["tested"]
    first_claim = int(np.argmax(t <= r32["eps"]))
    assert t[first_claim + 1] > 1e-10 * n0 and t[first_claim + 1] < 1e-6 * n0


@pytest.mark.parametrize("kdim,tol,precond,flexible", [(20, 1e-8, False, False), (5, 1e-10, True, False), (30, 1e-10, True, True)])
def test_without_rounding_it_is_the_existing_restatement(kdim, tol, precond, flexible):
    A, _, B = _laplace(6)
    b = np.random.default_rng(3).standard_normal(A.shape[0])
    kw = dict(tol=tol, kdim=kdim, max_iter=200, flexible=flexible)
    mine = ref.gmres(A, b, M=ref.dense_precond(B) if precond else None, rounding=False, **kw)
    theirs = kr.gmres(A, b, M=kr.dense_precond(B) if precond else None, **kw)
    assert mine["iters"] == theirs["iters"] and mine["converged"] == theirs["converged"] and mine["code"] == theirs["code"]
    assert len(mine["norms"]) == len(theirs["norms"])
    assert np.all(np.abs(mine["norms"] - theirs["norms"]) <= 1e-12 * theirs["norms"] + 1e-16 * theirs["norms"][0])
    assert np.abs(mine["x"] - theirs["x"]).max() <= 1e-12 * np.abs(theirs["x"]).max()
    assert len(mine["tested"]) == len(theirs["tested"]) and np.allclose(mine["tested"], theirs["tested"], rtol=1e-12,
                                                                     atol=1e-16 * theirs["norms"][0])


# ------------------------------------------------------------------ the cases of the device test
@pytest.fixture(scope="module")
def runs(oc):
    """every case in longdouble and in float64 with one Gram-Schmidt pass; the oracle's default cycle, tabulated"""
    tab, out = {}, {}
    for c in bc.CASES + bc.TURNED_AWAY:
        B = None
        if c["amg"]:
            if c["op"] not in tab:
                A = bc.operator(c["op"])
                amg = oc.Amg(oc.Csr.from_scipy(A), oc.default_params())
                e = np.zeros(A.shape[0])
                cols = []
                for j in range(A.shape[0]):
                    e[j] = 1.0
                    cols.append(amg.cycle(e))
                    e[j] = 0.0
                tab[c["op"]] = np.array(cols).T
            B = tab[c["op"]]
        out[c["id"]] = (bc.reference(c, B), bc.reference(c, B, arith="float64"))
    return out


def test_history_bar_is_the_measured_one(runs):
    """over the cases the device test runs (bc.CASES), and over those alone"""
    dev = {c["id"]: bc.history_deviation(*runs[c["id"]]) for c in bc.CASES}
    for cid, d in dev.items():
        print(f"{cid}: longdouble against float64 with one MGS pass, largest history deviation / ||r_0|| = {d:.3e}")
    worst = max(dev.values())
    print(f"ten times the largest: {10 * worst:.3e}; HISTORY_BAR = {bc.HISTORY_BAR:.3e}")
    assert bc.HISTORY_BAR / 1.05 <= 10 * worst <= bc.HISTORY_BAR


def test_the_listed_cases_qualify(runs):
    """the longdouble run alone decides: every tested value further from eps than the bar"""
    for cid, (ld, _) in runs.items():
        m = bc.margin(ld)
        print(f"{cid}: {ld['iters']} iterations, smallest |tested - eps| / ||r_0|| = {m:.3e}")
        assert ld["converged"]
        assert (m > bc.HISTORY_BAR) == (cid in bc.QUALIFYING), (cid, m)
    assert len(bc.QUALIFYING) >= 4 and [c["id"] for c in bc.TURNED_AWAY] == ["lap8_gmres5_restarts"]
    for cid in bc.RESTARTING:
        assert cid in bc.QUALIFYING and runs[cid][0]["iters"] > bc.by_id(cid)["kdim"]
    assert any(bc.by_id(cid)["ncomp"] == 3 for cid in bc.QUALIFYING)
    for cid in bc.QUALIFYING:  # and the double-precision run of the same steps agrees in its count
        assert runs[cid][1]["iters"] == runs[cid][0]["iters"]


# ------------------------------------------------------------------ ABI
NEW_SYMBOLS = ("HYPRE_MI_SetKrylovBasisStorage", "HYPRE_MI_GetKrylovBasisStorage", "HYPRE_MI_VectorKernelOpF32")


def test_new_symbols_are_declared_and_exported(mi_lib):
    from tests.test_abi import _declared_symbols

    names = _declared_symbols()
    lib = mi_lib.lib()
    for n in NEW_SYMBOLS:
        assert n in names and hasattr(lib, n), n
    assert callable(mi_lib.set_basis_storage) and callable(mi_lib.get_basis_storage)


def test_setting_round_trip_and_refusals(mi_lib):
    """0, 1, 2 are taken; -1 and 3 are refused with HYPRE_ERROR_ARG and leave the mode; no device needed"""
    before = mi_lib.get_basis_storage()
    try:
        for mode in (1, 2, 0, 2):
            mi_lib.set_basis_storage(mode)
            assert mi_lib.get_basis_storage() == mode
        for bad in (-1, 3):
            rc = mi_lib.call("HYPRE_MI_SetKrylovBasisStorage", bad, allow=(mi_lib.HYPRE_ERROR_ARG,))
            assert rc == mi_lib.HYPRE_ERROR_ARG
            assert b"SetKrylovBasisStorage" in mi_lib.lib().HYPRE_MI_LastErrorMessage()
            assert mi_lib.get_basis_storage() == 2
            mi_lib.call("HYPRE_ClearAllErrors")
    finally:
        mi_lib.set_basis_storage(before)


def test_an_environment_value_that_is_no_mode_is_reported(tmp_path):
    """MI_HYPRE_BASIS_STORAGE is read once per process: 7 (or a typo) leaves mode 0 and says so on stderr; 2 is taken"""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); import __graft_entry__ as ge; mi = ge.load_binding(); "
            "print('MODE', mi.get_basis_storage())" % root)
    for value, mode, warned in (("7", 0, True), ("fp32", 0, True), ("2", 2, False), ("", 0, False)):
        p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MI_HYPRE_BASIS_STORAGE=value),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert p.returncode == 0 and f"MODE {mode}" in p.stdout, (value, p.stdout, p.stderr)
        assert ("MI_HYPRE_BASIS_STORAGE=%s is not a mode" % value in p.stderr) == warned, (value, p.stderr)
