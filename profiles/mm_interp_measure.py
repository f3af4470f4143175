#!/usr/bin/env python3
"""Measurements of the matrix-matrix extended interpolations (interp_type 16 / 17) beside the default, type 6, in one
session on one device:
  sizes   -- bench.py --gpus 1 --steps 10 --warmup 2 --amg interp_type=T for T = 6, 16, 17 at every grid size, under
             MI_HYPRE_SETUP_TIMING=1: iterations, ms per solve, setup_s, operator complexity, levels, and the
             interpolation phase of the hierarchy build;
  default -- the default path (no override: type 6) with this build and with another build of the library (the parent
             commit's, through MI_HYPRE_LIB), alternating, `rounds` times: ms per solve and setup_s of every run and
             the spread (max - min) / min of each side.
Every bench run is a child process with its own time limit; the script stops at the first run that fails.
Usage: python profiles/mm_interp_measure.py [--sizes 256 512] [--types 6 16 17] [--parent-lib PATH] [--rounds 3] [--ab-size 512] [--out FILE]"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench(n, amg=None, lib=None, limit=420):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "2", "--n", str(n)]
    if amg:
        cmd += ["--amg", amg]
    env = dict(os.environ, MI_HYPRE_SETUP_TIMING="1")
    if lib:
        env["MI_HYPRE_LIB"] = lib
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit)
    if p.returncode != 0:
        raise SystemExit("bench.py failed (%d):\n%s" % (p.returncode, p.stdout[-3000:]))
    res = None
    for line in p.stdout.splitlines():
        if line.startswith("{") and '"value"' in line:
            res = json.loads(line)
    phases = re.findall(r"hierarchy build \(wall per phase\): strength ([\d.]+)\s+pmis ([\d.]+)\s+interp ([\d.]+)\s+galerkin ([\d.]+)"
                        r"\s+ordering/slicing ([\d.]+)\s+total ([\d.]+)", p.stdout)
    if res is None or not phases:
        raise SystemExit("bench.py printed no result line or no phase line:\n%s" % p.stdout[-3000:])
    res["interp_phase_s"], res["hierarchy_s"] = float(phases[0][2]), float(phases[0][5])  # (the first Setup: the build)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[256, 512])
    ap.add_argument("--types", type=int, nargs="*", default=[6, 16, 17],
                    help="interp_type values in the order they run (the first process at a size pays a cold start)")
    ap.add_argument("--parent-lib", default=None, help="libmi_hypre.so of the parent commit (skips the A/B part when absent)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ab-size", type=int, default=512)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say("bench.py --gpus 1 --steps 10 --warmup 2 --n N --amg interp_type=T, MI_HYPRE_SETUP_TIMING=1 (7-point Laplacian, "
        "GMRES(50) to 1e-8, P_max_elmts 4)")
    say("%5s %4s %6s %12s %9s %10s %16s %7s %8s" % ("n", "type", "iters", "ms/solve", "setup_s", "interp_s", "op. complexity", "levels", "GDOF/s"))
    for n in args.sizes:
        for t in args.types:
            r = bench(n, "interp_type=%d" % t)
            say("%5d %4d %6d %12.2f %9.3f %10.3f %16.4f %7d %8.3f" % (n, t, r["iterations_per_solve"], r["ms_per_step"], r["setup_s"],
                                                                     r["interp_phase_s"], r["operator_complexity"], r["amg_levels"], r["value"]))
    if args.parent_lib:
        say("")
        say("default path (no override) at %d^3: this build and the parent commit's library (MI_HYPRE_LIB), alternating" % args.ab_size)
        runs = {"parent": [], "this": []}
        for k in range(args.rounds):
            for side, lib in (("parent", os.path.abspath(args.parent_lib)), ("this", None)):
                r = bench(args.ab_size, lib=lib)
                runs[side].append(r)
                say("round %d %-6s: %d iterations, %.2f ms/solve, setup %.3f s (interp %.3f s), %.3f GDOF/s"
                    % (k, side, r["iterations_per_solve"], r["ms_per_step"], r["setup_s"], r["interp_phase_s"], r["value"]))
        for side in ("parent", "this"):
            for key, unit in (("ms_per_step", "ms/solve"), ("setup_s", "setup s")):
                v = [r[key] for r in runs[side]]
                say("%-6s %-9s min %.3f max %.3f spread %.2f %%" % (side, unit, min(v), max(v), 100.0 * (max(v) - min(v)) / min(v)))
        assert len({r["iterations_per_solve"] for side in runs for r in runs[side]}) == 1, "iteration counts differ"


if __name__ == "__main__":
    main()
