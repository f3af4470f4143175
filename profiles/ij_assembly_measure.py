"""Wall time of an IJ assembly from device-pointer triples: first HYPRE_IJMatrixSetValues2 to the end of
HYPRE_IJMatrixAssemble, for the 7-point operator at n^3 (row order, or shuffled with --shuffle).  One process per run;
the library is the one MI_HYPRE_LIB names (profiles/ab_ij_assembly.sh alternates two builds).  The triples are made
with torch on the device, the same for every build.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def triples(n, shuffle):
    N = n ** 3
    idx = torch.arange(N, dtype=torch.int64, device="cuda")
    x, y, z = idx % n, (idx // n) % n, idx // (n * n)
    offs = torch.tensor([-n * n, -n, -1, 0, 1, n, n * n], dtype=torch.int64, device="cuda")
    ok = torch.stack([z > 0, y > 0, x > 0, torch.ones_like(x, dtype=torch.bool), x < n - 1, y < n - 1, z < n - 1], dim=1)
    del x, y, z
    cols = (idx[:, None] + offs[None, :])[ok]
    rows = idx[:, None].expand(N, 7)[ok]
    vals = torch.where(offs == 0, 6.0, -1.0).to(torch.float64)[None, :].expand(N, 7)[ok]
    del ok, idx
    if shuffle:
        g = torch.Generator(device="cuda")
        g.manual_seed(1)
        p = torch.randperm(len(rows), device="cuda", generator=g)
        rows, cols, vals = rows[p].contiguous(), cols[p].contiguous(), vals[p].contiguous()
        del p
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return rows, cols, vals


def counter(mi, name):
    v = mi.C.c_longlong()
    rc = mi.lib().HYPRE_MI_GetCounter(name.encode(), mi.C.byref(v))
    if rc:
        mi.call("HYPRE_ClearAllErrors")
        return None
    return v.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--shuffle", action="store_true")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    mi = ge.load_binding()
    mi.init()
    N = a.n ** 3
    A = mi.IJMatrix(0, N - 1)
    rows, cols, vals = triples(a.n, a.shuffle)
    t0 = time.perf_counter()
    A.set_values_ptr(len(vals), rows.data_ptr(), cols.data_ptr(), vals.data_ptr())
    t1 = time.perf_counter()
    A.assemble()
    t2 = time.perf_counter()
    out = dict(label=a.label, n=a.n, shuffled=a.shuffle, entries=len(vals), set_values_s=round(t1 - t0, 3),
               assemble_s=round(t2 - t1, 3), total_s=round(t2 - t0, 3),
               arena_peak_in_use_bytes=counter(mi, "arena_peak_in_use_bytes"),
               device_assemblies=counter(mi, "ij_device_assemblies"), fetched=counter(mi, "ij_entries_fetched_to_host"))
    for k in ("kernels", "mirror", "format"):
        us = counter(mi, f"ij_last_{k}_us")
        out[f"{k}_s"] = None if us is None else round(us * 1e-6, 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
