#!/usr/bin/env python3
"""Unknown-based systems AMG (boomeramg num_functions; DESIGN.md section 3, "Systems of PDEs") beside the scalar setup
on coupled PDE systems, on one device.  The matrices are built here with numpy (COO triples, interleaved unknowns):
  lame    -- -mu Lap u - (lam + mu) grad div u on an n^3 grid by second-order finite differences, Dirichlet
             boundaries: 15 entries per interior row (7 of the row's component, 4 of each of the two others);
  fields  -- k diffusion fields on an n^3 grid (7-point; field a with diffusivities 1 + a, 1, 1 / (1 + a) along x, y,
             z), every pair coupled at every node by the exchange term c (u_a - u_b).
Every case runs with num_functions 1 and with num_functions k: two Setups of the same handle (the first pays the cold
start; the SECOND is reported), then one GMRES(50) solve to 1e-8 from x = 0 with b = A 1.  Reported per run: levels,
operator complexity, iterations, setup seconds, and -- from the library's MI_HYPRE_SETUP_TIMING lines of the second
Setup -- the seconds of the same-function filter and of strength() on its result, summed over the levels the device
built and for level 0.  A failing run ends the script.
Usage: python profiles/systems_amg_measure.py [--lame 48 64] [--fields 64] [--out FILE]"""
import argparse
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def grid(n):
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    return x.ravel(), y.ravel(), z.ravel()


def shifted(n, c, d):
    """nodes whose neighbour at offset d = (dx, dy, dz) lies in the grid, and that neighbour"""
    ok = np.ones(n ** 3, dtype=bool)
    for a in range(3):
        ok &= (c[a] + d[a] >= 0) & (c[a] + d[a] < n)
    p = np.flatnonzero(ok)
    return p, p + d[0] + n * d[1] + n * n * d[2]


def lame_triples(n, lam, mu):
    """(rows, cols, vals) of the interleaved system: unknown a of node p is row 3 p + a"""
    c = grid(n)
    R, C, V = [], [], []
    e = np.eye(3, dtype=int)
    nodes = np.arange(n ** 3)
    for a in range(3):
        R.append(3 * nodes + a), C.append(3 * nodes + a), V.append(np.full(n ** 3, 6.0 * mu + 2.0 * (lam + mu)))
        for b in range(3):
            w = -mu - (lam + mu if a == b else 0.0)  # -mu Lap u_a, and -(lam + mu) d_a d_a u_a
            for s in (-1, 1):
                p, q = shifted(n, c, s * e[b])
                R.append(3 * p + a), C.append(3 * q + a), V.append(np.full(len(p), w))
            if b == a:
                continue
            for sa in (-1, 1):  # -(lam + mu) d_a d_b u_b, central differences: -+ (lam + mu) / 4 at the four corners
                for sb in (-1, 1):
                    p, q = shifted(n, c, sa * e[a] + sb * e[b])
                    R.append(3 * p + a), C.append(3 * q + b), V.append(np.full(len(p), -(lam + mu) * 0.25 * sa * sb))
    return np.concatenate(R), np.concatenate(C), np.concatenate(V)


def field_triples(n, k, coupling):
    c = grid(n)
    R, C, V = [], [], []
    e = np.eye(3, dtype=int)
    nodes = np.arange(n ** 3)
    for a in range(k):
        diff = (1.0 + a, 1.0, 1.0 / (1.0 + a))
        R.append(k * nodes + a), C.append(k * nodes + a), V.append(np.full(n ** 3, 2.0 * sum(diff) + coupling * (k - 1)))
        for b in range(3):
            for s in (-1, 1):
                p, q = shifted(n, c, s * e[b])
                R.append(k * p + a), C.append(k * q + a), V.append(np.full(len(p), -diff[b]))
        for o in range(k):
            if o != a:
                R.append(k * nodes + a), C.append(k * nodes + o), V.append(np.full(n ** 3, -coupling))
    return np.concatenate(R), np.concatenate(C), np.concatenate(V)


def flush_c():
    import ctypes

    ctypes.CDLL(None).fflush(None)


def run_case(mi, label, triples, k, amg_kw, say):
    rows, cols, vals = triples
    N = int(rows.max()) + 1
    A = mi.IJMatrix(0, N - 1)
    A.set_values_coo(rows.astype(np.int64), cols.astype(np.int64), vals.astype(np.float64))
    A.assemble()
    rhs = np.bincount(rows, weights=vals, minlength=N)  # A 1
    for nf in (1, k):
        amg = mi.BoomerAMG(print_level=0, num_functions=nf, **amg_kw)
        amg.setup(A)
        flush_c()  # (the library's lines sit in C stdio's buffer when stdout is a pipe: keep them between the markers)
        print("SECOND SETUP %s nf=%d" % (label, nf), flush=True)
        amg.setup(A)
        setup_s = amg.setup_seconds
        flush_c()
        print("END SETUP", flush=True)
        b, x = mi.IJVector(0, N - 1, rhs), mi.IJVector(0, N - 1, np.zeros(N))
        gm = mi.GMRES(tolerance=1e-8, max_iterations=200, kspace=50, print_level=0)
        gm.set_precond(amg)
        gm.setup(A, b, x)  # (the preconditioner is set up: a third Setup of the same kind)
        t0 = time.time()
        rc = gm.solve(A, b, x)
        solve_s = time.time() - t0
        err = float(np.abs(x.get() - 1.0).max())
        say("RUN %-34s rows %8d nf %d levels %2d opcx %.3f iters %3d rc %d setup_s %.3f solve_s %.3f max|x-1| %.1e"
            % (label, N, nf, amg.num_levels, amg.operator_complexity, gm.num_iterations, rc, setup_s, solve_s, err))


def worker(args):
    import __graft_entry__ as ge

    mi = ge.load_binding()
    mi.init()
    say = lambda s: print(s, flush=True)
    for n in args.lame:
        for lam in (1.0, 10.0):
            tr = lame_triples(n, lam, 1.0)
            for theta in (0.25, 0.5):
                run_case(mi, "lame n=%d lam=%g theta=%g" % (n, lam, theta), tr, 3, dict(strong_threshold=theta), say)
    for n in args.fields:
        for coupling in (0.1, 10.0):
            run_case(mi, "fields n=%d k=2 c=%g theta=0.25" % (n, coupling), field_triples(n, 2, coupling), 2,
                     dict(strong_threshold=0.25), say)


def table(out):
    """the report from the worker's output: its RUN lines and the library's timing lines of every second Setup"""
    lines = ["unknown-based systems AMG beside the scalar setup: second of two Setups, GMRES(50) to 1e-8, b = A 1",
             "filter / strength: seconds of the same-function filter and of strength() on F(A) in that Setup, summed over the levels the device built (level 0)",
             "%-34s %8s %2s %6s %6s %5s %8s %8s %18s %18s %7s" % ("case", "rows", "nf", "levels", "opcx", "iters", "setup_s", "solve_s",
                                                                   "filter_s (l0)", "strength_s (l0)", "ratio")]
    block, blocks = None, {}
    for line in out:
        m = re.match(r"SECOND SETUP (.*) nf=(\d+)", line)
        if m:
            block = (m.group(1), int(m.group(2)))
            blocks[block] = []
        elif line.startswith("END SETUP"):
            block = None
        elif block is not None:
            blocks[block].append(line)
        m = re.match(r"RUN (.*?) +rows +(\d+) nf (\d+) levels +(\d+) opcx ([\d.]+) iters +(\d+) rc (\d+) setup_s ([\d.]+) solve_s ([\d.]+)", line)
        if m:
            label, nf = m.group(1).strip(), int(m.group(3))
            ft = [(int(a), float(b), float(c)) for a, b, c in
                  re.findall(r"level (\d+): n \d+  same-function filter ([\d.]+) s, strength ([\d.]+) s$", "\n".join(blocks.get((label, nf), [])), re.M)]
            f_all, s_all = sum(t[1] for t in ft), sum(t[2] for t in ft)
            f0, s0 = (ft[0][1], ft[0][2]) if ft else (0.0, 0.0)
            lines.append("%-34s %8s %2d %6s %6s %5s %8s %8s %18s %18s %7s"
                         % (label, m.group(2), nf, m.group(4), m.group(5), m.group(6) + ("" if m.group(7) == "0" else "*"), m.group(8),
                            m.group(9), "%.4f (%.4f)" % (f_all, f0) if ft else "-", "%.4f (%.4f)" % (s_all, s0) if ft else "-",
                            "%.2f" % (f_all / s_all) if ft and s_all > 0 else "-"))
    text = "\n".join(lines) + "\n(* = GMRES did not reach the tolerance in 200 iterations)\n"
    return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lame", type=int, nargs="*", default=[48, 64])
    ap.add_argument("--fields", type=int, nargs="*", default=[64])
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    # the library prints its phase lines on the process's stdout: run the cases in a child and read both streams there
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--lame"] + [str(n) for n in args.lame] + ["--fields"] + \
          [str(n) for n in args.fields]
    env = dict(os.environ, MI_HYPRE_SETUP_TIMING="1", PYTHONUNBUFFERED="1")
    p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out = []
    for line in p.stdout:  # (the runs are shown as they finish)
        out.append(line.rstrip("\n"))
        if line.startswith("RUN "):
            print(line, end="", flush=True)
    if p.wait() != 0:
        raise SystemExit("the worker failed (%d):\n%s" % (p.returncode, "\n".join(out[-60:])))
    text = table(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
