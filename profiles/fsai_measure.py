"""FSAI measurements recorded in DESIGN.md section 9 (one GPU, 7-point Laplacian):
  setup   -- HYPRE_FSAISetup on the n^3 operator for fsai_num_levels k = 1, 2 (wall time, synchronised);
  sweeps  -- relaxation time per GMRES iteration on levels 0 and 1 (HIP-event classes 20 + l: every launch of the
             level's down and up sweep) with FSAI on levels 0-1 against the default l1-hybrid-GS (relax_type 8);
  solve   -- GMRES(50) to 1e-8 with BoomerAMG: the default, FSAI on levels 0-1, FSAI on every level (refused when a
             coarse level's pattern exceeds 64 entries in a row): iterations, setup, solve.
With --adaptive the same for the adaptive pattern (fsai_algo_type 4) at its defaults -- setup beside the static k = 1,
the three solves, G's size and the rows that took the table in global memory (HYPRE_MI_FSAIGetSetupInfo /
HYPRE_MI_BoomerAMGGetLevelFSAIInfo).
Usage: python profiles/fsai_measure.py [--sizes 256 512] [--skip-solve] [--adaptive] [--out results.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def gmres(mi, A, b, x, amg):
    x.fill(0.0)
    gm = mi.GMRES(tolerance=1e-8, max_iterations=200, kspace=50, print_level=0)
    gm.set_precond(amg)
    t0 = time.perf_counter()
    gm.setup(A, b, x)
    t1 = time.perf_counter()
    gm.solve(A, b, x)  # warm
    x.fill(0.0)
    t2 = time.perf_counter()
    gm.solve(A, b, x)
    t3 = time.perf_counter()
    return gm, t1 - t0, t3 - t2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--skip-solve", action="store_true")
    ap.add_argument("--adaptive", action="store_true", help="also measure fsai_algo_type 4 at its defaults")
    ap.add_argument("--out", default=None, help="also write the results as JSON to this file")
    args = ap.parse_args()
    mi = ge.load_binding()
    mi.init()
    out = {}
    for n in args.sizes:
        A, b, x, rhs = mi.build_laplace_system(n, n, n, 7)
        rec = {}
        for k in (1, 2):
            times = []
            for rep in range(2):
                fs = mi.FSAI(num_levels=k)
                t0 = time.perf_counter()
                fs.setup(A)
                times.append(time.perf_counter() - t0)
                fs.destroy()
            rec[f"fsai_setup_s_k{k}"] = times
        if args.adaptive:
            times = []
            for rep in range(2):
                fs = mi.FSAI(algo_type=4)
                t0 = time.perf_counter()
                fs.setup(A)
                times.append(time.perf_counter() - t0)
                rec["fsai_adaptive_info"] = fs.setup_info()
                fs.destroy()
            rec["fsai_setup_s_adaptive"] = times
        if not args.skip_solve:
            configs = [("default", {}), ("fsai_levels_0_1", dict(smooth_type=4, smooth_num_levels=2)),
                       ("fsai_all_levels", dict(smooth_type=4, smooth_num_levels=50))]
            if args.adaptive:
                configs += [("adaptive_levels_0_1", dict(smooth_type=4, smooth_num_levels=2, fsai_algo_type=4)),
                            ("adaptive_all_levels", dict(smooth_type=4, smooth_num_levels=50, fsai_algo_type=4))]
            for name, kw in configs:
                amg = mi.BoomerAMG(print_level=0, **kw)
                try:
                    gm, ts, tsol = gmres(mi, A, b, x, amg)
                except mi.HypreError as e:  # e.g. a coarse level whose FSAI pattern exceeds 64 entries in a row
                    rec[name] = dict(error=str(e))
                    mi.call("HYPRE_ClearAllErrors")
                    amg.destroy()
                    continue
                r = dict(iterations=gm.num_iterations, setup_s=ts, solve_s=tsol, rel_res=gm.final_rel_res)
                if kw.get("fsai_algo_type") == 4:
                    r["level_fsai_info"] = [amg.level_fsai_info(lev)
                                            for lev in range(min(kw["smooth_num_levels"], amg.num_levels - 1))]
                for lev in (0, 1):
                    mi.profile_enable(20 + lev, 1 << 16)
                mi.profile_reset()
                x.fill(0.0)
                gm.solve(A, b, x)
                for lev in (0, 1):
                    launches, total, mn = mi.profile_get(20 + lev)
                    r[f"level{lev}_relax_ms_per_iteration"] = total / max(gm.num_iterations, 1)
                    r[f"level{lev}_relax_launches"] = launches
                rec[name] = r
                amg.destroy()
        out[n] = rec
        print(json.dumps({n: rec}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
