"""GMRES and COGMRES behind a level-ordered BoomerAMG: the update from the kept directions z_j = M^-1 p_j against the
recomputed update of gmres.c (HYPRE_MI_SetGmresKeepDirections 1 / 0), on the cases of tests/kept_directions_cases.py.

For every case both paths run and
  1. iterations, return code and residual history are equal bit for bit (the Arnoldi process is shared; the history
     comes from the Givens data);
  2. "precond_cycles" per solve is iterations x components with the kept directions and (iterations + solution
     updates) x components without (a multivector is cycled component by component);
  3. each path meets the project's bounds against the restatement (krylov_gpu_common.check_against_reference: x within
     1e-9 max|x_ref|, history within 1e-7 |r| + 1e-13 r0, the final relative residual), and the two x agree within the
     same 1e-9 max|x_ref|.
One component: the kept vector adopts the level-0 solution buffer of the cycle (pointer swap); three components: the
copy path.  Further: solver objects used again (adopted buffers leak nothing between solves), the history under
print_level 2, a kept vector that cannot be allocated (test hook), and the guards -- without a preconditioner, with
the preconditioner set up on another matrix object and with MI_HYPRE_GMRES_PERMUTED=0 the switch changes no bit and no
direction vector is allocated."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import kept_directions_cases as kd
from tests import krylov_cases as kc
from tests import krylov_gpu_common as kg
from tests import krylov_ref as kr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_MATS, _TAB, _REF = {}, {}, {}


def matrix(mi, op):
    if op not in _MATS:
        _MATS[op] = mi.matrix_from_scipy(kd.operator(op))
    return _MATS[op]


def tabulated_amg(mi, op):
    """the library's default BoomerAMG cycle on an operator as a dense map, once per operator and module"""
    if op not in _TAB:
        A = matrix(mi, op)
        n = kd.operator(op).shape[0]
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


def reference(mi, solver, case):
    """the restatement's answer (gmres.c's update), once per case and module"""
    key = kc.case_id((solver, case))
    if key not in _REF:
        A, b, x0 = kd.system(case)
        _REF[key] = kc.reference(solver, case, A, b, x0, kr.dense_precond(tabulated_amg(mi, case["op"])))
    return _REF[key]


def counted(mi, fn):
    """(fn(), preconditioner cycles it ran, direction vectors it allocated)"""
    c0, z0 = mi.counter("precond_cycles"), mi.counter("gmres_direction_vectors")
    out = fn()
    return out, mi.counter("precond_cycles") - c0, mi.counter("gmres_direction_vectors") - z0


def run(mi, solver, case, keep, amg=True, A_solve=None, print_level=0):
    """a fresh solver (and a fresh BoomerAMG) on a case with the switch at `keep`"""
    A, b, x0 = kd.system(case)
    s = kg.make_solver(mi, solver, case)
    if print_level:
        mi.call(f"{s.prefix}SetPrintLevel", s.h, print_level)
    if amg:
        s.set_precond(mi.BoomerAMG(print_level=0))
    mi.set_gmres_keep_directions(keep)
    try:
        Am = matrix(mi, case["op"])
        return counted(mi, lambda: kg.solve(mi, s, A_solve if A_solve is not None else Am, b, x0, A_setup=Am))
    finally:
        mi.set_gmres_keep_directions(True)


def same_process(a, b):
    return a["code"] == b["code"] and a["iters"] == b["iters"] and a["hist"].tobytes() == b["hist"].tobytes()


@pytest.mark.parametrize("sc", kd.ALL, ids=kc.case_id)
def test_both_paths(mi, sc):
    solver, case = sc
    nc, kdim = case["ncomp"], case["kdim"]
    ref = reference(mi, solver, case)
    _, b, x0 = kd.system(case)
    kept, cyc_kept, z_kept = run(mi, solver, case, True)
    rec, cyc_rec, z_rec = run(mi, solver, case, False)
    dx = float(np.abs(kept["x"] - rec["x"]).max())
    print(f"{kc.case_id(sc)}: {kept['iters']} iterations, cycles {cyc_kept} kept / {cyc_rec} recomputed, "
          f"max|x_kept - x_recomputed| = {dx:.3e} = {dx / np.abs(ref['x']).max():.3e} max|x|, rel res "
          f"{kept['rel']:.6e} / {rec['rel']:.6e}")
    assert same_process(kept, rec)
    m = kept["iters"]
    assert cyc_kept == m * nc, (cyc_kept, m, nc)
    assert cyc_rec == (m + kd.updates(m, kdim)) * nc, (cyc_rec, m, kdim, nc)
    assert z_kept == min(m, kdim) and z_rec == 0, (z_kept, z_rec)
    kg.check_against_reference(kept, ref, solver, b, x0)
    kg.check_against_reference(rec, ref, solver, b, x0)
    assert dx <= kd.x_bound(ref["x"]), (dx, kd.x_bound(ref["x"]))
    if case["max_iter"] < 200:
        assert kept["code"] == 256 and m == case["max_iter"] and m % kdim != 0  # x from a partial basis


def test_history_does_not_depend_on_print_level(mi, capfd):
    solver, case = kd.RESTARTS[0]
    quiet, _, _ = run(mi, solver, case, True)
    loud, _, _ = run(mi, solver, case, True, print_level=2)
    capfd.readouterr()
    assert kg.same_bits(quiet, loud) and len(quiet["hist"]) == quiet["iters"] + 1


@pytest.mark.parametrize("sc", [kd.BASE[2], kd.RESTARTS[0]], ids=kc.case_id)
def test_solver_object_used_again(mi, sc):
    """One GMRES object and one BoomerAMG: the case, the case again, another right-hand side and guess, the case again.
    Every answer equals a fresh pair's bit for bit: the buffers the kept vectors adopted and handed back carry nothing
    from one solve (or cycle) into the next."""
    solver, case = sc
    A, b, x0 = kd.system(case)
    _, b2, x02 = kd.system(case, seed=77)
    Am = matrix(mi, case["op"])
    one = kg.make_solver(mi, solver, case)
    one.set_precond(mi.BoomerAMG(print_level=0))
    fresh = {id(b): run(mi, solver, case, True)[0]}
    s2 = kg.make_solver(mi, solver, case)
    s2.set_precond(mi.BoomerAMG(print_level=0))
    fresh[id(b2)] = kg.solve(mi, s2, Am, b2, x02)
    for step, (bb, xx) in enumerate(((b, x0), (b, x0), (b2, x02), (b, x0))):
        got = kg.solve(mi, one, Am, bb, xx, setup=step == 0)
        assert got["iters"] > 5 and kg.same_bits(got, fresh[id(bb)]), step


@pytest.mark.parametrize("sc,at", [(kd.BASE[3], 2), (kd.RESTARTS[1], 1), (kd.BASE[3], 0)],
                         ids=["cd9_third_vector", "cd9_k3_second_vector", "cd9_first_vector"])
def test_no_room_for_a_kept_vector(mi, sc, at):
    """The allocation of kept vector number `at` fails (test hook): nothing is raised, the restart cycle under way and
    the rest of the solve take the recomputed update -- bit for bit the answer with the switch off -- and only the
    vectors before it were allocated."""
    solver, case = sc
    rec, cyc_rec, _ = run(mi, solver, case, False)
    mi.call("HYPRE_MI_TestGmresDirectionAllocFailsAt", at)
    try:
        got, cyc, z = run(mi, solver, case, True)
    finally:
        mi.call("HYPRE_MI_TestGmresDirectionAllocFailsAt", -1)
    assert kg.same_bits(got, rec) and cyc == cyc_rec and z == at, (cyc, cyc_rec, z)


def test_guards_in_this_process(mi):
    """No preconditioner, and a Solve on another matrix object than the preconditioner's Setup saw (natural order): the
    switch changes nothing bit for bit and no direction vector is allocated."""
    plain = kc.make_case("plain", "cd7")
    a, cyc_a, z_a = run(mi, "gmres", plain, True, amg=False)
    b, cyc_b, z_b = run(mi, "gmres", plain, False, amg=False)
    assert kg.same_bits(a, b) and (cyc_a, z_a, cyc_b, z_b) == (0, 0, 0, 0)
    solver, case = kd.RESTARTS[1]
    A2 = mi.matrix_from_scipy(kd.operator(case["op"]))
    a, cyc_a, z_a = run(mi, solver, case, True, A_solve=A2)
    b, cyc_b, z_b = run(mi, solver, case, False, A_solve=A2)
    m = a["iters"]
    assert kg.same_bits(a, b) and z_a == 0 and z_b == 0
    assert cyc_a == cyc_b == m + kd.updates(m, case["kdim"]), (cyc_a, cyc_b, m)


def _child(**env):
    e = dict(os.environ, **{k: str(v) for k, v in env.items()})
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "kept_directions_worker.py")],
                       env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_guard_natural_order_process(mi):
    """MI_HYPRE_GMRES_PERMUTED=0 in a child process: BoomerAMG through its Solve entry point, the recomputed update
    whatever the switch says."""
    solver, case = kd.RESTARTS[1]
    out = _child(MI_HYPRE_GMRES_PERMUTED=0)
    on, off = kg.from_json(out["on"]), kg.from_json(out["off"])
    m = on["iters"]
    assert kg.same_bits(on, off) and out["z_on"] == 0 and out["z_off"] == 0
    assert out["cycles_on"] == out["cycles_off"] == m + kd.updates(m, case["kdim"])
    _, b, x0 = kd.system(case)
    kg.check_against_reference(on, reference(mi, solver, case), solver, b, x0)


def test_environment_switch(mi):
    """MI_HYPRE_GMRES_KEEP_DIRECTIONS=0 in a child process is the setter at 0: the child's run with the switch left
    alone equals this process's recomputed run bit for bit, and the setter still turns the feature on there."""
    solver, case = kd.RESTARTS[1]
    out = _child(MI_HYPRE_GMRES_KEEP_DIRECTIONS=0)
    rec, cyc_rec, _ = run(mi, solver, case, False)
    kept, cyc_kept, _ = run(mi, solver, case, True)
    assert kg.same_bits(kg.from_json(out["default"]), rec) and out["cycles_default"] == cyc_rec and out["z_default"] == 0
    assert kg.same_bits(kg.from_json(out["on"]), kept) and out["cycles_on"] == cyc_kept
