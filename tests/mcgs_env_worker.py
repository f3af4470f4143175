"""The multicolour Gauss-Seidel checks that depend on switches the library reads once per process
(tests/test_gpu_mcgs.py starts this program once per setting and compares the printed results):
  dict   MI_HYPRE_VALUE_DICT: sweeps of type 40 / 41 / 42 on level 0 of the constant 27-point stencil at 15^3, the value
         format of that level and the instantiation that ran
  tail   MI_HYPRE_DENSE_TAIL_ROWS: one cycle (down 40, up 41, dense coarsest solve) on the 7-point operator at 12^3"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def device_matrix(mi, M):
    A = mi.IJMatrix(0, M.shape[0] - 1)
    coo = M.tocoo()
    A.set_values_coo(coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data.astype(np.float64))
    A.assemble()
    return A


def dictionary(mi):
    from tests import mcgs_cases as cases

    M = cases.case("constant_stencil")
    A = device_matrix(mi, M)
    amg = mi.BoomerAMG(print_level=0, down_relax_type=40, up_relax_type=41, coarse_relax_type=42)
    amg.setup(A)
    n = M.shape[0]
    rng = np.random.default_rng(6)
    f, u = rng.standard_normal(n), rng.standard_normal(n)
    out = {"kind": amg.level_value_storage(0, 0)[0]}
    mi.profile_enable(mi.PROF_LVL_RELAX_MC)
    for t in (40, 41, 42):
        out[str(t)] = amg.relax_level(0, t, 0, f, u).tobytes().hex()
    out["kernel"] = mi.profile_kernel_name(mi.PROF_LVL_RELAX_MC)
    return out


def tail(mi):
    from tests import mcgs_cases as cases

    M = cases.laplace(12, 7)
    n = M.shape[0]
    A = device_matrix(mi, M)
    amg = mi.BoomerAMG(print_level=0, down_relax_type=40, up_relax_type=41, coarse_relax_type=9)
    amg.setup(A)
    f = np.random.default_rng(7).standard_normal(n)
    fi, ui = mi.IJVector(0, n - 1, f), mi.IJVector(0, n - 1, np.zeros(n))
    amg.solve(A, fi, ui)  # max_iterations 1, tolerance 0: exactly one cycle
    return {"x": ui.get().tobytes().hex(), "levels": amg.num_levels}


def main():
    mi = ge.load_binding()
    mi.init()
    print("RESULT " + json.dumps({"dict": dictionary, "tail": tail}[sys.argv[1]](mi)), flush=True)


if __name__ == "__main__":
    main()
