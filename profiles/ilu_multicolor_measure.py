"""Multicolour ordering of the ILU (local_reordering 2) against the natural ordering (0): the measurements recorded in
DESIGN.md section 9 (one GPU, n^3 Laplacians, ILU(0) with exact triangular solves).  Per case and ordering:
  setup   -- HYPRE_ILUSetup wall time, synchronised, second of two setups; colours, rounds, level sets per factor;
  step    -- one HYPRE_ILUSolve step x += M^-1 (b - A x) (max_iterations 1: one residual SpMV, one application of the
             factors, one axpy), HIP events on the library's stream: after a warm-up step a pilot window of --reps
             steps sizes --windows windows of at least --window-s seconds each; reported are the median window's
             milliseconds per step and the smallest and largest window (the spread).  The launches of the
             application itself are its level sets (one launch each) plus, with the ordering, one scatter --
             counted from the setup's report, not observed;
  precond -- GMRES(50) to --tol with the ILU as preconditioner: iterations, seconds per solve (second of two solves);
  smooth  -- the same GMRES with BoomerAMG whose level 0 carries the ILU as complex smoother (smooth_type 5,
             smooth_num_levels 1, ilu_reordering_type 0 / 2): AMG setup seconds, iterations, seconds per solve.
Usage: python profiles/ilu_multicolor_measure.py [--cases 128:7 128:27 256:7 256:27] [--tol 1e-8] [--out results.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


class Events:
    """two HIP events on the library's stream"""

    def __init__(self, mi):
        self.hip = mi.lib()  # the HIP runtime the library is linked against resolves through its handle
        self.stream = C.c_void_p()
        mi.call("HYPRE_MI_GetStream", C.byref(self.stream))
        self.e = [C.c_void_p(), C.c_void_p()]
        for e in self.e:
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def record(self, which):
        assert self.hip.hipEventRecord(self.e[which], self.stream) == 0

    def elapsed_ms(self):
        assert self.hip.hipEventSynchronize(self.e[1]) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.e[0], self.e[1]) == 0
        return float(ms.value)


def gmres(mi, A, b, x, precond, tol, maxit):
    gm = mi.GMRES(tolerance=tol, max_iterations=maxit, kspace=50, print_level=0)
    gm.set_precond(precond)
    x.fill(0.0)
    t0 = time.perf_counter()
    gm.setup(A, b, x)
    mi.call("HYPRE_MI_StreamSynchronize")
    setup_s = time.perf_counter() - t0
    gm.solve(A, b, x)  # warm
    x.fill(0.0)
    mi.call("HYPRE_MI_StreamSynchronize")
    t0 = time.perf_counter()
    gm.solve(A, b, x)
    mi.call("HYPRE_MI_StreamSynchronize")
    r = dict(krylov_setup_s=setup_s, iterations=gm.num_iterations, solve_s=time.perf_counter() - t0,
             rel_res=gm.final_rel_res)
    gm.destroy()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["128:7", "128:27", "256:7", "256:27"], help="n:stencil")
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--maxit", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=10, help="steps of the pilot window")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--window-s", type=float, default=0.5, help="least length of a timed window")
    ap.add_argument("--skip-smooth", action="store_true")
    ap.add_argument("--out", default=None, help="also write the results as JSON to this file")
    args = ap.parse_args()
    mi = ge.load_binding()
    mi.init()
    ev = Events(mi)
    out = {}
    for case in args.cases:
        n, stencil = (int(v) for v in case.split(":"))
        A, b, x, rhs = mi.build_laplace_system(n, n, n, stencil)
        for reordering in (0, 2):
            times = []
            for rep in range(2):
                ilu = mi.ILU(max_iterations=1, tolerance=0.0, trisolve=1, local_reordering=reordering)
                mi.call("HYPRE_MI_StreamSynchronize")
                t0 = time.perf_counter()
                ilu.setup(A)
                mi.call("HYPRE_MI_StreamSynchronize")
                times.append(time.perf_counter() - t0)
                if rep == 0:
                    ilu.destroy()
            o = ilu.ordering()
            r = dict(setup_s=times[1], setup_first_s=times[0], **{k: o[k] for k in mi.ILU_ORDERING_NAMES})
            r["apply_launches"] = o["lower_levels"] + o["upper_levels"] + (1 if o["reordering"] else 0)
            x.fill(0.0)
            ilu.solve(A, b, x)  # warm

            def window(steps):
                ev.record(0)
                for _ in range(steps):
                    ilu.solve(A, b, x)
                ev.record(1)
                return ev.elapsed_ms() / steps

            steps = max(args.reps, int(1000.0 * args.window_s / window(args.reps)) + 1)
            ms = sorted(window(steps) for _ in range(args.windows))
            r.update(step_ms=ms[len(ms) // 2], step_ms_min=ms[0], step_ms_max=ms[-1], steps_per_window=steps)
            r["precond"] = gmres(mi, A, b, x, ilu, args.tol, args.maxit)
            ilu.destroy()
            if not args.skip_smooth:
                amg = mi.BoomerAMG(print_level=0, smooth_type=5, smooth_num_levels=1, ilu_reordering_type=reordering)
                r["smooth"] = gmres(mi, A, b, x, amg, args.tol, 200)
                r["smooth"]["amg_setup_s"] = amg.setup_seconds
                amg.destroy()
            out.setdefault(case, {})[f"reordering{reordering}"] = r
            print(json.dumps({case: {f"reordering{reordering}": r}}), flush=True)
            if args.out:
                with open(args.out, "w") as f:
                    json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
