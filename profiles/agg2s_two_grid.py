"""Two-grid factors of an aggressive first level: two-stage extended interpolation (agg_interp_type 5) beside multipass
(4) on the library's own splitting, one symmetric Gauss-Seidel sweep as smoother, dense algebra -- the figure of
profiles/r03_two_grid_aggressive.txt.  Host-only setup (no GPU needed).  Appends to profiles/agg2s_two_grid.txt:
    python profiles/agg2s_two_grid.py 12 16"""
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from tests.agg2s_common import two_grid_factor  # noqa: E402


def main():
    mi = ge.load_binding()
    mi.lib()
    with open(os.path.join(ROOT, "profiles", "agg2s_two_grid.txt"), "a") as out:
        measure(mi, out, [int(a) for a in sys.argv[1:]] or [12])


def measure(mi, out, sizes):
    for n in sizes:
        A, _ = mi.build_laplace_system_host(n, n, n, 7, 0, 1)
        for label, kw in (("multipass (4)", dict(agg_interp_type=4)),
                          ("two-stage extended (5), no truncation", dict(agg_interp_type=5)),
                          ("two-stage extended (5), agg_pmax_elmts 4", dict(agg_interp_type=5, agg_pmax_elmts=4)),
                          ("two-stage extended (5), agg_pmax_elmts 4, agg_p12_max_elmts 4",
                           dict(agg_interp_type=5, agg_pmax_elmts=4, agg_p12_max_elmts=4))):
            amg = mi.BoomerAMG(print_level=0, agg_num_levels=1, **kw)
            mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
            ia, ja, a, shape = amg.level_csr(0, 0)
            pia, pja, pa, pshape = amg.level_csr(0, 2)
            rho = two_grid_factor(sp.csr_matrix((a, ja, ia), shape=shape), sp.csr_matrix((pa, pja, pia), shape=pshape))
            line = "7-pt %d^3  %-62s C points %5d  entries per row of P %.2f  two-grid factor %.4f" % (
                n, label, pshape[1], len(pa) / pshape[0], rho)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
