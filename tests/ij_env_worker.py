"""Device IJ assembly in a process of its own, for the switches that are read once per process
(tests/test_gpu_ij_device_assembly.py::test_switches_in_a_child_process): the shuffled 7-point 12^3 triples and a
GMRES + BoomerAMG solve of a 16^3 system, each from device arrays and from numpy arrays; prints whether the two agree
bit for bit, and the counters."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from tests import ij_cases as cases  # noqa: E402


def solve(mi, n, device):
    N = n ** 3
    A = cases.new_matrix(mi, 0, N - 1)
    cases.stage(mi, A, [cases.laplace_triples(mi, n, 7) + (False,)], device)
    A.assemble()
    b = mi.IJVector(0, N - 1, np.cos(np.arange(N, dtype=np.float64)))
    x = mi.IJVector(0, N - 1, np.zeros(N))
    amg = mi.BoomerAMG(print_level=0)
    gm = mi.GMRES(tolerance=1e-9, max_iterations=60, kspace=50, print_level=0)
    gm.set_precond(amg)
    gm.setup(A, b, x)
    assert gm.solve(A, b, x) == 0
    return gm.num_iterations, gm.residual_history().view(np.int64), x.get().view(np.int64)


def main():
    mi = ge.load_binding()
    mi.init()
    r, c, v = cases.laplace_triples(mi, 12, 7)
    p = np.random.default_rng(5).permutation(len(v))
    batch = (r[p].copy(), c[p].copy(), v[p].copy(), False)
    snaps = []
    for device in (True, False):
        A = cases.new_matrix(mi, 0, 12 ** 3 - 1)
        cases.stage(mi, A, [batch], device)
        A.assemble()
        snaps.append(cases.snapshot(mi, A))
        A.destroy()
    shuffled_equal = bool(cases.same(*snaps))
    d, h = solve(mi, 16, True), solve(mi, 16, False)
    solve_equal = d[0] == h[0] and np.array_equal(d[1], h[1]) and np.array_equal(d[2], h[2])
    print("RESULT " + json.dumps({"shuffled_equal": shuffled_equal, "solve_equal": bool(solve_equal), "iters": d[0],
                                  "device_assemblies": mi.counter("ij_device_assemblies"),
                                  "fetched": mi.counter("ij_entries_fetched_to_host"),
                                  "entries": len(v) + len(cases.laplace_triples(mi, 16, 7)[2])}))


if __name__ == "__main__":
    main()
