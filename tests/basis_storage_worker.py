"""Child process of tests/test_gpu_basis_storage.py, for the switches that are read once per process
(MI_HYPRE_GMRES_PERMUTED, MI_HYPRE_POISON_ALLOC): the solves named on the command line (tests/basis_storage_gpu_common.py)
under basis storage modes 1 and 2.  Prints "RESULT {id: [digest under mode 1, digest under mode 2, iterations]}"; a
digest covers the iteration count, the residual history, x and the final relative residual."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from tests import basis_storage_gpu_common as bg  # noqa: E402


def main():
    mi = ge.load_binding()
    mi.init()
    systems = bg.Systems(mi)
    out = {}
    for sid in sys.argv[1:]:
        spec = bg.by_id(sid)
        r1, r2 = systems.run(spec, 1), systems.run(spec, 2)
        out[sid] = [bg.digest(r1), bg.digest(r2), r1["iters"]]
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
