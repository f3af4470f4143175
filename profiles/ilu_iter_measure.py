"""Iterative ILU(0) setup measurements recorded in DESIGN.md section 9 (one GPU, HYPRE_ILU as GMRES preconditioner):
  setup  -- HYPRE_ILUSetup wall time (synchronised, second of two setups) for type 0 (exact, level-scheduled) and
            types 3, 4, 1 with 1, 5 and 20 sweeps, each with trisolve 0 (Jacobi triangular solves) and 1 (exact);
  sweeps -- sweeps of type 3 until the correction c <= 1e-5 (option bits 2 | 4), and the residual after them;
  solve  -- GMRES(50) to --tol with the ILU preconditioner: iterations and time per solve (second of two solves).
Kernel statistics: run under `rocprofv3 --kernel-trace --stats -- python profiles/ilu_iter_measure.py --skip-solve`.
Usage: python profiles/ilu_iter_measure.py [--cases 256:7 128:27] [--skip-solve] [--tol 1e-6] [--out results.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def settings():
    yield "type0", dict()
    for typ in (3, 4, 1):
        for sweeps in (1, 5, 20):
            yield f"type{typ}_sweeps{sweeps}", dict(iterative_algorithm_type=typ, iterative_max_iterations=sweeps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["256:7", "128:27"], help="n:stencil")
    ap.add_argument("--skip-solve", action="store_true")
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--maxit", type=int, default=1000)
    ap.add_argument("--out", default=None, help="also write the results as JSON to this file")
    args = ap.parse_args()
    mi = ge.load_binding()
    mi.init()
    out = {}
    for case in args.cases:
        n, stencil = (int(v) for v in case.split(":"))
        A, b, x, rhs = mi.build_laplace_system(n, n, n, stencil)
        rec = {}
        ilu = mi.ILU(iterative_algorithm_type=3, iterative_setup_option=2 | 4 | 8, iterative_max_iterations=200,
                     iterative_tolerance=1e-5, trisolve=0)
        ilu.setup(A)
        sw, c, r = ilu.iterative_setup_info()
        rec["type3_sweeps_to_c_1e-5"] = dict(sweeps=sw, correction=c, residual=r)
        ilu.destroy()
        for name, kw in settings():
            for tri in (0, 1):
                times = []
                for rep in range(2):
                    ilu = mi.ILU(trisolve=tri, **kw)
                    t0 = time.perf_counter()
                    ilu.setup(A)
                    times.append(time.perf_counter() - t0)
                    if rep == 0:
                        ilu.destroy()
                r = dict(setup_s=times[1], setup_first_s=times[0])
                if not args.skip_solve:
                    gm = mi.GMRES(tolerance=args.tol, max_iterations=args.maxit, kspace=50, print_level=0)
                    gm.set_precond(ilu)
                    x.fill(0.0)
                    gm.setup(A, b, x)
                    gm.solve(A, b, x)  # warm
                    x.fill(0.0)
                    t0 = time.perf_counter()
                    gm.solve(A, b, x)
                    r.update(iterations=gm.num_iterations, solve_s=time.perf_counter() - t0, rel_res=gm.final_rel_res)
                    gm.destroy()
                ilu.destroy()
                rec[f"{name}_trisolve{tri}"] = r
                print(json.dumps({case: {f"{name}_trisolve{tri}": r}}), flush=True)
        out[case] = rec
        if args.out:
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
