"""Wall time of giving an assembled IJ matrix new values from device-pointer triples, 7-point operator at n^3 (row
order, or shuffled with --shuffle).  One process per run; the library is the one MI_HYPRE_LIB names.
  --mode update  an update round: first HYPRE_IJMatrixSetValues2 on the assembled matrix to the end of
                 HYPRE_IJMatrixAssemble, split into kernels / value dictionary / host mirror by the library's counters;
  --mode fresh   the only way without update rounds (the parent commit): Destroy, Create and a full device assembly of
                 the same triples.
Both start from a matrix that was assembled once (untimed) and hand over the same new values.  Prints one JSON line;
profiles/ij_value_update.sh alternates the two and wrote profiles/ij_value_update.txt."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from profiles.ij_assembly_measure import counter, triples  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--mode", choices=["update", "fresh"], default="update")
    ap.add_argument("--shuffle", action="store_true")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    mi = ge.load_binding()
    mi.init()
    N = a.n ** 3
    rows, cols, vals = triples(a.n, a.shuffle)
    A = mi.IJMatrix(0, N - 1)
    A.set_values_ptr(len(vals), rows.data_ptr(), cols.data_ptr(), vals.data_ptr())
    A.assemble()
    peak_first = counter(mi, "arena_peak_in_use_bytes")
    vals = (1.5 * vals).contiguous()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if a.mode == "fresh":
        A.destroy()
        A = mi.IJMatrix(0, N - 1)
    A.set_values_ptr(len(vals), rows.data_ptr(), cols.data_ptr(), vals.data_ptr())
    t1 = time.perf_counter()
    A.assemble()
    t2 = time.perf_counter()
    out = dict(label=a.label, mode=a.mode, n=a.n, shuffled=a.shuffle, entries=len(vals), set_values_s=round(t1 - t0, 3),
               assemble_s=round(t2 - t1, 3), total_s=round(t2 - t0, 3), arena_peak_after_first_assembly=peak_first,
               arena_peak_after_round=counter(mi, "arena_peak_in_use_bytes"),
               device_value_updates=counter(mi, "ij_device_value_updates"), device_assemblies=counter(mi, "ij_device_assemblies"))
    names = ("update_kernels", "update_dictionary", "update_mirror") if a.mode == "update" else ("last_kernels", "last_mirror", "last_format")
    for k in names:
        us = counter(mi, f"ij_{k}_us")
        out[f"{k}_s"] = None if us is None else round(us * 1e-6, 3)
    # the updated matrix is usable: a product with ones gives the scaled row sums (0 inside the cube)
    x = mi.IJVector(0, N - 1)
    x.fill(1.0)
    y = mi.IJVector(0, N - 1)
    mi.call("HYPRE_ParCSRMatrixMatvec", 1.0, A.par, x.par, 0.0, y.par)
    out["row_sum_max"] = float(abs(y.get()).max())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
