"""Device setup of operators of tests/systems.py (INTERP_TABLE_OPERATORS) in a process of its own, for the switches that
are read once per process (tests/test_gpu_interp_tables.py runs it with MI_HYPRE_POISON_ALLOC=1): prints a digest of
every level's A, P, R, marks and ordering per job.  Arguments: name:interp_type:true_pmax_elmts ..."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from tests.systems import INTERP_TABLE_OPERATORS, interp_table_operator  # noqa: E402


def hierarchy_digest(amg):
    h = hashlib.sha256()
    for l in range(amg.num_levels):
        for which in (0, 2, 3) if l < amg.num_levels - 1 else (0,):
            for arr in amg.level_csr(l, which)[:3]:
                h.update(np.ascontiguousarray(arr).tobytes())
        if l < amg.num_levels - 1:
            h.update(amg.level_cf(l).tobytes() + amg.level_perm(l).tobytes())
    return h.hexdigest()


def main():
    mi = ge.load_binding()
    mi.init()
    out = {}
    for job in sys.argv[1:]:
        name, interp, pmax = job.split(":")
        A = mi.matrix_from_scipy(interp_table_operator(name)[0])
        amg = mi.BoomerAMG(print_level=0, strong_threshold=INTERP_TABLE_OPERATORS[name][1], interp_type=int(interp),
                           true_pmax_elmts=int(pmax))
        amg.setup(A)
        out[job] = dict(digest=hierarchy_digest(amg), census=amg.interp_census(0))
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
