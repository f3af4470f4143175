"""Chebyshev relaxation (relax_type 16) against the default l1 symmetric Gauss-Seidel (relax_type 8), the numbers of
DESIGN.md section 9 (one GPU, 7-point Laplacian n^3):
  driver -- hypre_app on etc/laplace_3d_cheby.yaml at n^3 for orders 2 and 3 and on the relax_type 8 input: iterations,
            setup seconds, seconds per solve (the driver's own timer summary is kept in the raw output);
  level0 -- HIP-event class 20 (level-0 relaxation): one Chebyshev step against one l1-SGS C/F pair, and the step's
            achieved bandwidth against its byte count (matrix stream + 5 vector reads + 2 vector writes per row).
Usage: python profiles/cheby_measure.py [--n 256] [--out results.txt]"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

APP = os.path.join(ROOT, "hypre-mini-app_amd", "hypre_app")
YAML = os.path.join(ROOT, "hypre-mini-app_amd", "etc", "laplace_3d_cheby.yaml")


def driver(n, relax_type, order, lines):
    text = re.sub(r"(n[xyz]): 64", r"\1: %d" % n, open(YAML).read())
    text = text.replace("relax_type: 16", "relax_type: %d" % relax_type)
    if relax_type == 16:
        text += "  mi_cheby_order: %d\n" % order
    with tempfile.TemporaryDirectory() as d:
        inp = os.path.join(d, "input.yaml")
        open(inp, "w").write(text)
        t0 = time.perf_counter()
        p = subprocess.run([APP, inp], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        wall = time.perf_counter() - t0
    name = "relax_type %d" % relax_type + (" order %d" % order if relax_type == 16 else "")
    lines.append("---- hypre_app %d^3, %s (rc %d, wall %.1f s)" % (n, name, p.returncode, wall))
    keep = re.compile(r"iterations|setup|Setup|solve|Solve|Total time|max \|x", re.I)
    lines.extend("   " + l for l in p.stdout.splitlines() if keep.search(l))


def level0(mi, n, lines):
    A, b, x, rhs = mi.build_laplace_system(n, n, n, 7)
    pid = mi.PROF_LVL_RELAX
    for name, kw in (("l1-SGS (relax_type 8), C/F pair", dict(relax_type=8, relax_order=1)),
                     ("Chebyshev order 2", dict(relax_type=16, cheby_order=2)),
                     ("Chebyshev order 3", dict(relax_type=16, cheby_order=3))):
        amg = mi.BoomerAMG(print_level=0, **kw)
        gm = mi.GMRES(tolerance=1e-8, max_iterations=200, kspace=50, print_level=0)
        gm.set_precond(amg)
        x.fill(0.0)
        t0 = time.perf_counter()
        gm.setup(A, b, x)
        t1 = time.perf_counter()
        gm.solve(A, b, x)  # warm
        x.fill(0.0)
        mi.profile_enable(pid)
        mi.profile_reset()
        t2 = time.perf_counter()
        gm.solve(A, b, x)
        t3 = time.perf_counter()
        launches, total_ms, min_ms = mi.profile_get(pid)
        nrows = n ** 3
        nnz = 7 * nrows - 6 * n * n
        kind, vbytes = amg.level_value_storage(0, 0)
        # the matrix stream: the value bytes as stored, 2-byte tile-local columns, 4-byte row pointers
        stream = vbytes + 2 * nnz + 4 * nrows
        line = "%-34s: %3d iterations, setup %.3f s, solve %.4f s; level-0 relax class: %d launches, mean %.4f ms, min %.4f ms" % (
            name, gm.num_iterations, t1 - t0, t3 - t2, launches, total_ms / max(launches, 1), min_ms)
        if kw["relax_type"] == 16:
            nbytes = stream + 7 * 8 * nrows
            line += "; step bytes %.3f GB (value kind %d) -> %.2f TB/s at the minimum" % (nbytes / 1e9, kind, nbytes / (min_ms * 1e-3) / 1e12)
        lines.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    driver(args.n, 8, 0, lines)
    driver(args.n, 16, 2, lines)
    driver(args.n, 16, 3, lines)
    mi = ge.load_binding()
    mi.init()
    level0(mi, args.n, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
