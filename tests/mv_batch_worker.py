"""One GMRES(20) + BoomerAMG solve of the 3-component convection-diffusion system in a process of its own, with the
multivector batch width given on the command line, for the switches that are read once per process
(tests/test_gpu_multivector_batch.py: MI_HYPRE_GMRES_PERMUTED, MI_HYPRE_POISON_ALLOC).  Prints the iteration count, the
residual history and the solution as hex, and the multivector counters."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from tests.systems import convection_diffusion_3d, three_component_rhs  # noqa: E402


def main():
    width = int(sys.argv[1])
    mi = ge.load_binding()
    mi.init()
    mi.set_multivector_batch(width)
    M = convection_diffusion_3d(12)
    B, _ = three_component_rhs(M)
    N = M.shape[0]
    A = mi.matrix_from_scipy(M)
    b = mi.IJVector(0, N - 1, B, ncomp=3)
    x = mi.IJVector(0, N - 1, np.zeros((3, N)), ncomp=3)
    amg = mi.BoomerAMG(print_level=0)
    gm = mi.GMRES(tolerance=1e-9, max_iterations=60, kspace=20, print_level=0)
    gm.set_precond(amg)
    gm.setup(A, b, x)
    assert gm.solve(A, b, x) == 0
    print("RESULT " + json.dumps({"iters": gm.num_iterations, "hist": [float(h).hex() for h in gm.residual_history()],
                                  "x": x.get_all().tobytes().hex(),
                                  "counters": {k: mi.counter(k) for k in ("mv_batched_cycles", "mv_batched_matvecs",
                                                                         "mv_fallback_cycles", "precond_cycles")}}))


if __name__ == "__main__":
    main()
