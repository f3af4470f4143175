"""The multicolour ordering and the ILU(0) factors behind it on the named cases of tests/ilu_color_cases.py: digest()
returns what two runs can compare exactly.  As a program it runs in a process of its own, for the library switches that
are read once per process (MI_HYPRE_POISON_ALLOC; tests/test_gpu_ilu_color.py), and prints the digest."""
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def ij(mi, M):
    M = sp.csr_matrix(M)
    n = M.shape[0]
    A = mi.IJMatrix(0, n - 1)
    coo = M.tocoo()
    A.set_values_coo(coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data.astype(np.float64))
    A.assemble()
    return A


def digest(mi, names):
    from tests import ilu_color_cases as cc

    out = {}
    for name in names:
        M = cc.matrix(name)
        n = M.shape[0]
        A = ij(mi, M)
        ilu = mi.ILU(max_iterations=1, tolerance=0.0, local_reordering=2)
        ilu.setup(A)
        o = ilu.ordering()
        ia, ja, a = ilu.factors()
        b = mi.IJVector(0, n - 1, M @ np.ones(n))
        x = mi.IJVector(0, n - 1, np.zeros(n))
        ilu.solve(A, b, x)
        out[name] = dict(info=[o[k] for k in mi.ILU_ORDERING_NAMES], perm=o["perm"].tolist(), colour=o["colour"].tolist(),
                         ia=ia.tolist(), ja=ja.tolist(), a=a.tobytes().hex(), x=x.get().tobytes().hex())
        ilu.destroy()
    return out


def main():
    mi = ge.load_binding()
    mi.init()
    print("RESULT " + json.dumps(digest(mi, sys.argv[1:])))


if __name__ == "__main__":
    main()
