"""Cases of tests/krylov_cases.py in a process of its own, for the library switches that are read once per process
(tests/test_gpu_krylov_paths.py).  Modes:
  amg     the BoomerAMG-preconditioned cases (MI_HYPRE_GMRES_PERMUTED=0: the natural-order path)
  vec     the vector-kernel checks at every length (MI_HYPRE_VEC_BLOCKS=2: up to five grid-stride trips), then `solves`
  solves  the converging unpreconditioned GMRES and COGMRES cgs 2 cases (MI_HYPRE_GMRES_POLL=0 against the polled run)
Prints the results as hex so that two runs can be compared bit for bit."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from tests import krylov_cases as kc  # noqa: E402
from tests import krylov_gpu_common as kg  # noqa: E402


def main():
    mode = sys.argv[1]
    mi = ge.load_binding()
    mi.init()
    out = {}
    if mode == "amg":
        A = mi.matrix_from_scipy(kc.operator("cd9"))
        amg = mi.BoomerAMG(print_level=0)
        for solver, case in kc.AMG:
            out[kc.case_id((solver, case))] = kg.to_json(kg.run_case(mi, solver, case, A, amg=amg))
    else:
        if mode == "vec":
            for n in kg.VEC_N:
                kg.check_vector_kernels(mi, n)
        A = mi.matrix_from_scipy(kc.operator("cd7"))
        for solver in ("gmres", "cogmres2"):
            out[kc.case_id((solver, kc.NOPRECOND[0]))] = kg.to_json(kg.run_case(mi, solver, kc.NOPRECOND[0], A))
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
