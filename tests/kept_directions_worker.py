"""The restarted BoomerAMG-preconditioned GMRES case of tests/kept_directions_cases.py in a process of its own, for the
switches that are read once per process (MI_HYPRE_GMRES_PERMUTED, MI_HYPRE_GMRES_KEEP_DIRECTIONS;
tests/test_gpu_gmres_kept_directions.py): the solve with the switch as the environment left it ("default"), then with
HYPRE_MI_SetGmresKeepDirections at 1 and at 0.  Prints the results as hex, with the preconditioner cycles and the
direction vectors each solve counted."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from tests import kept_directions_cases as kd  # noqa: E402
from tests import krylov_gpu_common as kg  # noqa: E402


def main():
    mi = ge.load_binding()
    mi.init()
    solver, case = kd.RESTARTS[1]
    A, b, x0 = kd.system(case)
    Am = mi.matrix_from_scipy(A)
    out = {}
    for name, keep in (("default", None), ("on", True), ("off", False)):
        if keep is not None:
            mi.set_gmres_keep_directions(keep)
        s = kg.make_solver(mi, solver, case)
        s.set_precond(mi.BoomerAMG(print_level=0))
        c0, z0 = mi.counter("precond_cycles"), mi.counter("gmres_direction_vectors")
        out[name] = kg.to_json(kg.solve(mi, s, Am, b, x0))
        out["cycles_" + name] = mi.counter("precond_cycles") - c0
        out["z_" + name] = mi.counter("gmres_direction_vectors") - z0
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
