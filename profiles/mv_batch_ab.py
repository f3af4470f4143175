"""Multivector batch, A/B in one process: the 3-component convection-diffusion system (tests/systems.py) at n^3, GMRES(50)
+ BoomerAMG and BiCGSTAB + BoomerAMG with default settings, HYPRE_MI_SetMultivectorBatch(1) against (4) -- three
components share a pass -- alternating, `--reps` solves each after one warm-up solve of each, profiler off.  Then one
solve of each width with the profile classes of the fine levels on: milliseconds per launch of the level-0 mat-vec and of
the relaxation / residual / restriction / prolongation passes of levels 0 .. 3 (a batched launch serves three components,
a looped one a single component: compare 3 x looped against batched).

Bytes per row of level 0 (7-point operator): the matrix streams are about 90 B without a value
dictionary (72 B with the one-byte dictionary: 7 x (2 B column word + 8 B / 1 B value) + column list + descriptor + row
pointer), the vector traffic of one component about 55 B (gather at 0.72 unique columns per entry, f and u).  Three
components batched move (90 + 3 x 55) / (3 x 145) = 0.59 of the looped bytes (0.72 with the dictionary).

  python profiles/mv_batch_ab.py --n 128 [--reps 5]        prints one JSON line per (solver, width) and a summary"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from tests.systems import convection_diffusion_3d  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    mi = ge.load_binding()
    mi.init()
    M = convection_diffusion_3d(a.n)
    N = M.shape[0]
    rng = np.random.default_rng(99)
    B = np.stack([M @ rng.standard_normal(N) for _ in range(3)])
    A = mi.matrix_from_scipy(M)
    del M
    b = mi.IJVector(0, N - 1, B, ncomp=3)
    x = mi.IJVector(0, N - 1, np.zeros((3, N)), ncomp=3)
    summary = {}
    for solver in ("gmres", "bicgstab"):
        amg = mi.BoomerAMG(print_level=0)
        s = (mi.GMRES(tolerance=1e-8, max_iterations=200, kspace=50, print_level=0) if solver == "gmres" else
             mi.BiCGSTAB(tolerance=1e-8, max_iterations=200, print_level=0))
        s.set_precond(amg)
        s.setup(A, b, x)

        def solve(width):
            mi.set_multivector_batch(width)
            x.set_component(0)
            for c in range(3):
                x.set_component(c)
                x.fill(0.0)
            t0 = time.perf_counter()
            rc = s.solve(A, b, x)
            dt = time.perf_counter() - t0
            assert rc == 0, rc
            return dt, s.num_iterations, s.final_rel_res

        for width in (1, 4):
            solve(width)
        times = {1: [], 4: []}
        its = {}
        for _ in range(a.reps):
            for width in (1, 4):
                dt, it, rr = solve(width)
                times[width].append(dt)
                its[width] = (it, rr)
        assert its[1] == its[4], its  # the same bits: the same iteration count and residual
        for width in (1, 4):
            t = times[width]
            row = dict(n=a.n, solver=solver, width=width, iterations=its[width][0], median_s=statistics.median(t),
                       min_s=min(t), max_s=max(t), all_s=t)
            summary[solver, width] = row
            print("RESULT " + json.dumps(row), flush=True)
        # per class, one solve each
        pids = {"spmv_l0": mi.PROF_SPMV_L0}
        for lvl in range(4):
            pids.update({f"relax_l{lvl}": mi.PROF_LVL_RELAX + lvl, f"relax0_l{lvl}": mi.PROF_LVL_RELAX0 + lvl,
                         f"resid_l{lvl}": mi.PROF_LVL_RESID + lvl, f"restrict_l{lvl}": mi.PROF_LVL_RESTRICT + lvl,
                         f"prolong_l{lvl}": mi.PROF_LVL_PROLONG + lvl})
        for pid in pids.values():
            mi.profile_enable(pid, 1 << 14)
        for width in (1, 4):
            mi.profile_reset()
            solve(width)
            row = {}
            for name, pid in pids.items():
                launches, total_ms, _ = mi.profile_get(pid)
                if launches:
                    row[name] = dict(launches=launches, ms_per_launch=total_ms / launches, kernel=mi.profile_kernel_name(pid))
            print("CLASSES " + json.dumps(dict(n=a.n, solver=solver, width=width, classes=row)), flush=True)
        for pid in pids.values():
            mi.profile_enable(pid, 0)
    for solver in ("gmres", "bicgstab"):
        one, four = summary[solver, 1], summary[solver, 4]
        print(f"{solver} n={a.n}: width 1 median {one['median_s']:.4f} s [{one['min_s']:.4f}, {one['max_s']:.4f}]   "
              f"width 4 median {four['median_s']:.4f} s [{four['min_s']:.4f}, {four['max_s']:.4f}]   "
              f"ratio {four['median_s'] / one['median_s']:.3f}   ({one['iterations']} iterations)")


if __name__ == "__main__":
    main()
