#!/usr/bin/env python3
"""Table of the compiler's per-kernel resource remarks for the solve-phase kernels.

  hipcc -O3 -std=c++17 -Iinclude -Ihypre-mini-app_amd/csrc --offload-arch=gfx950 --cuda-device-only \
        -Rpass-analysis=kernel-resource-usage -S hypre-mini-app_amd/csrc/kernels.hip -o kernels.s 2> remarks.txt
  python profiles/resource_report.py remarks.txt [other_remarks.txt]

With two files (e.g. the parent commit's and this one's) the rows are matched by kernel name and printed side by side;
a kernel that exists in one file only has dashes in the other's columns.  Names are demangled with c++filt and cut
at the argument list.  A trailing default template argument (", false" / ", double") is dropped from the name so that
an instantiation keeps its row when a defaulted parameter is appended to its template.
"""
import re
import subprocess
import sys

KEYS = (("VGPRs", "vgpr"), ("TotalSGPRs", "sgpr"), ("ScratchSize [bytes/lane]", "scratch"),
        ("Occupancy [waves/SIMD]", "waves"), ("LDS Size [bytes/block]", "lds"))
WANTED = ("spmv_stream", "gs_tile_k", "gs_group_k", "gs_dense_k", "gs_hybrid_k", "two_stage_lower_k")


def parse(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        for key, short in KEYS:
            m = re.search(r"remark:\s+" + re.escape(key) + r": (\d+)", line)
            if m and cur:
                out[cur][short] = int(m.group(1))
    names = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True).stdout.split("\n")
    table = {}
    for mangled, name in zip(out, names):
        name = re.sub(r"^void ", "", name)
        name = re.sub(r"\(.*$", "", name.replace("mi::k::(anonymous namespace)::", ""))
        name = re.sub(r", (false|double)>$", ">", name).replace("<double>", "")
        if any(w in name for w in WANTED):
            table[name] = out[mangled]
    return table


def main():
    tabs = [parse(p) for p in sys.argv[1:3]]
    names = sorted(set().union(*tabs))
    head = "%-46s" % "kernel" + "".join("  | " + " ".join("%7s" % s for _, s in KEYS) for _ in tabs)
    print(head)
    for n in names:
        row = "%-46s" % n
        for t in tabs:
            row += "  | " + " ".join("%7s" % (t[n][s] if n in t else "-") for _, s in KEYS)
        print(row)


if __name__ == "__main__":
    main()
