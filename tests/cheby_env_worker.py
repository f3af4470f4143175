"""GMRES(10) and PCG with BoomerAMG relax type 16 on the 7-point 12^3 problem, every order, both eigenvalue estimates,
V and W cycles: solve_matrix() checks convergence and the true residual and returns a digest that two runs can compare
bit for bit.  As a program it runs in a process of its own, for the library switches that are read once per process
(tests/test_gpu_cheby.py), and prints the digest."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

N = 12
# the solvers stop on their recurrence residual; the recomputed one differs from it by O(eps * condition number), far
# below this margin
TRUE_RES = 1e-8 * (1.0 + 1e-6)


def solve_matrix(mi, orders=(1, 2, 3, 4), ests=(0, 10), cycles=(1, 2), solvers=("gmres", "pcg")):
    from tests.test_cheby_spec import laplace

    A, b, x, rhs = mi.build_laplace_system(N, N, N, 7)
    L = laplace(N)
    out = {}
    for est in ests:
        for cyc in cycles:
            for order in orders:
                for name in solvers:
                    amg = mi.BoomerAMG(print_level=0, relax_type=16, cheby_order=order, cheby_eig_est=est, cycle_type=cyc)
                    if name == "gmres":
                        ks = mi.GMRES(tolerance=1e-8, max_iterations=100, kspace=10, print_level=0)
                    else:
                        ks = mi.PCG(tolerance=1e-8, max_iterations=100, print_level=0, two_norm=1)
                    ks.set_precond(amg)
                    x.fill(0.0)
                    ks.setup(A, b, x)
                    rc = ks.solve(A, b, x)
                    xs = x.get()
                    key = f"{name} est{est} cycle{cyc} order{order}"
                    assert rc == 0 and ks.num_iterations <= 100, (key, rc, ks.num_iterations)
                    assert np.all(np.isfinite(xs)), key
                    res = np.linalg.norm(rhs - L @ xs) / np.linalg.norm(rhs)
                    assert res <= TRUE_RES, (key, res)
                    hist = np.asarray(ks.residual_history(), dtype=np.float64)
                    if name == "pcg":
                        # a preconditioner that is not symmetric shows as residuals that climb or stall
                        assert np.all(hist[1:] <= 1.5 * hist[:-1]), (key, hist)
                    out[key] = dict(iters=int(ks.num_iterations), x=xs.tobytes().hex(), hist=[float(h).hex() for h in hist])
    return out


def main():
    mi = ge.load_binding()
    mi.init()
    few = dict(orders=(2, 3), ests=(10,)) if len(sys.argv) > 1 and sys.argv[1] == "few" else {}
    print("RESULT " + json.dumps(solve_matrix(mi, **few)))


if __name__ == "__main__":
    main()
