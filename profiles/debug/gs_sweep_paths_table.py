"""Per level and pass of the benchmark hierarchy: which branch of the tile Gauss-Seidel kernel's in-chunk sweep the
waves take (host-side census, HYPRE_MI_BoomerAMGGetGSSweepPaths).   python3 profiles/debug/gs_sweep_paths_table.py 256
The census reads a host copy of each level operator: 12 bytes per entry (11 GB for level 0 at 512^3)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))  # repo root
import __graft_entry__ as ge

mi = ge.load_binding()
mi.init()
n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
A, b, x, _ = mi.build_laplace_system(n, n, n, 7, 0, 1)
amg = mi.BoomerAMG(print_level=0)
amg.setup(A)
print(f"laplace_3d {n}^3 7-pt, {amg.num_levels} levels; share of the launched waves per branch")
print(f"{'level':>5s} {'pass':28s} {'waves':>10s} {'idle %':>8s} {'diagonal %':>11s} {'zero-guess %':>13s} {'general %':>10s}")
for level in range(amg.num_levels - 1):
    for label, points, zero in (("zero-guess C pass", 1, True), ("zero-guess F pass", -1, True), ("C pass", 1, False),
                                ("F pass", -1, False)):
        c = amg.gs_sweep_paths(level, points, zero)
        if c is None:
            print(f"{level:5d} {label:28s} (not on the tile kernel)")
            continue
        w = max(c["waves"], 1)
        print(f"{level:5d} {label:28s} {c['waves']:10d} {100 * c['idle'] / w:8.1f} {100 * c['diagonal'] / w:11.1f} "
              f"{100 * c['zero'] / w:13.1f} {100 * c['general'] / w:10.1f}", flush=True)
