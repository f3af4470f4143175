"""Child process of tests/test_gpu_agg2s.py::test_nothing_reads_memory_it_has_not_written: builds a hierarchy with two
aggressive levels and the two-stage extended interpolation (agg_interp_type 5, both truncations) on the device, checks it
against the host-only setup bit for bit, and prints "RESULT <sha256>" over every level's operator, interpolation, C/F
marker and stage markers.  The parent compares the line between runs with different allocator settings."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from tests.agg2s_common import host_amg  # noqa: E402


def digest(amg, nagg):
    h = hashlib.sha256()
    for l in range(amg.num_levels):
        for which in (0, 2) if l < amg.num_levels - 1 else (0,):
            ia, ja, a, shape = amg.level_csr(l, which)
            for arr in (ia, ja, a):
                h.update(np.ascontiguousarray(arr).tobytes())
        if l < amg.num_levels - 1:
            h.update(np.ascontiguousarray(amg.level_cf(l)).tobytes())
        if l < min(nagg, amg.num_levels - 1):
            for m in amg.level_agg_markers(l):
                h.update(np.ascontiguousarray(m).tobytes())
    return h.hexdigest()


def main():
    mi = ge.load_binding()
    mi.init()
    n = 14
    kw = dict(agg_num_levels=2, agg_interp_type=5, agg_pmax_elmts=4, agg_p12_max_elmts=6, agg_p12_trunc_factor=0.05)
    A = mi.build_laplace_system(n, n, n, 27)[0]
    dev = mi.BoomerAMG(print_level=0, keep_agg_markers=1, **kw)
    dev.setup(A)
    host = host_amg(mi, mi.build_laplace_system_host(n, n, n, 27, 0, 1)[0], **kw)
    assert dev.num_levels == host.num_levels > 2
    d, hd = digest(dev, 2), digest(host, 2)
    assert d == hd, "device and host-only hierarchies differ"
    print("RESULT " + d, flush=True)


if __name__ == "__main__":
    main()
