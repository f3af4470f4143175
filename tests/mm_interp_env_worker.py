"""Child process of tests/test_gpu_mm_interp.py::test_nothing_reads_memory_it_has_not_written: builds hierarchies with the
matrix-matrix extended interpolations (interp_type 16 and 17, truncated) on the device, checks them against the
host-only setup bit for bit, and prints "RESULT <sha256>" over every level's operator, interpolation and C/F marker.
The parent compares the line between runs with different allocator settings."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from tests.agg2s_common import host_amg  # noqa: E402


def digest(h, amg):
    for l in range(amg.num_levels):
        for which in (0, 2) if l < amg.num_levels - 1 else (0,):
            ia, ja, a, shape = amg.level_csr(l, which)
            for arr in (ia, ja, a):
                h.update(np.ascontiguousarray(arr).tobytes())
        if l < amg.num_levels - 1:
            h.update(np.ascontiguousarray(amg.level_cf(l)).tobytes())


def main():
    mi = ge.load_binding()
    mi.init()
    n = 14
    hd, hh = hashlib.sha256(), hashlib.sha256()
    for t in (16, 17):
        kw = dict(interp_type=t, true_pmax_elmts=4, trunc_factor=0.05)
        A = mi.build_laplace_system(n, n, n, 27)[0]
        dev = mi.BoomerAMG(print_level=0, **kw)
        dev.setup(A)
        host = host_amg(mi, mi.build_laplace_system_host(n, n, n, 27, 0, 1)[0], **kw)
        assert dev.num_levels == host.num_levels > 2
        digest(hd, dev)
        digest(hh, host)
    assert hd.hexdigest() == hh.hexdigest(), "device and host-only hierarchies differ"
    print("RESULT " + hd.hexdigest(), flush=True)


if __name__ == "__main__":
    main()
