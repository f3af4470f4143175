"""Host-only AMG setup timing for profiles/level_build_refactor_timing.txt: the four phase columns of the line
"mi_hypre hierarchy build (wall per phase)" (MI_HYPRE_SETUP_TIMING=1, MI_HYPRE_HOST_THREADS=8) for the default settings,
aggressive multipass and agg_interp_type 5 on the 7-point Laplacian, five runs per case in one process.

  python profiles/level_build_host_timing.py --libs parent=<parent libmi_hypre.so> new=<this build's> [--sizes 64 96]

Without --libs it is the worker: it runs the cases with the library MI_HYPRE_LIB names and lets the library print."""
import argparse
import ctypes
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"default": {}, "agg_multipass": dict(agg_num_levels=1), "agg_interp_type_5": dict(agg_num_levels=1, agg_interp_type=5)}
PHASES = ("strength", "pmis", "interp", "galerkin")
RUNS = 5


def worker(n):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge

    mi = ge.load_binding()
    mi.lib()
    A = mi.build_laplace_system_host(n, n, n, 7, 0, 1)[0]
    for name, kw in CASES.items():
        for _ in range(RUNS):
            print("CASE %s" % name, flush=True)
            amg = mi.BoomerAMG(print_level=0, **kw)
            mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
            ctypes.CDLL(None).fflush(None)  # the library prints through C stdio: keep its lines under their CASE line


def measure(lib, n):
    env = dict(os.environ, MI_HYPRE_LIB=os.path.realpath(lib), MI_HYPRE_SETUP_TIMING="1", MI_HYPRE_HOST_THREADS="8")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", str(n)], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, check=True).stdout
    runs, case = {}, None
    for line in out.splitlines():
        if line.startswith("CASE "):
            case = line.split()[1]
        m = re.match(r"mi_hypre hierarchy build \(wall per phase\): strength ([\d.]+)  pmis ([\d.]+)  interp ([\d.]+)  galerkin ([\d.]+)", line)
        if m:
            runs.setdefault(case, []).append([float(v) for v in m.groups()])
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", type=int, default=0)
    ap.add_argument("--libs", nargs=2, metavar="NAME=PATH")
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 96])
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker)
    (pname, ppath), (nname, npath) = [x.split("=", 1) for x in args.libs]
    fmt = lambda v: " ".join("%.2f" % x for x in v)
    for n in args.sizes:
        print("n = %d (%d rows)" % (n, n ** 3))
        print("  %-18s %-9s %-30s median spread | %-30s median" % ("case", "phase", pname + " runs", nname + " runs"))
        res = {pname: measure(ppath, n), nname: measure(npath, n)}
        for case in CASES:
            for k, phase in enumerate(PHASES):
                a = [r[k] for r in res[pname][case]]
                b = [r[k] for r in res[nname][case]]
                ma, mb, spread = statistics.median(a), statistics.median(b), max(a) - min(a)
                flag = "" if mb <= ma + spread + 1e-9 else "   (*) above the parent's median + spread"
                print("  %-18s %-9s %-30s %.2f   %.2f   | %-30s %.2f%s" % (case, phase, fmt(a), ma, spread, fmt(b), mb, flag))


if __name__ == "__main__":
    main()
