"""One rank of the multi-rank iterative ILU(0) check (launched by torch.distributed.run from tests/test_gpu_itilu.py):
ranks sharing the GPU, each with a slice of a 3-D Laplacian.  Every rank's type-3 factors must equal the numpy sweeps
on its own diagonal block bit for bit, the type-1 factors the exact ILU(0) of the block, GMRES with the iterative ILU
preconditioner and (without an empty rank) BoomerAMG with iterative ILU smoothers must converge.  --empty 1: the last
rank owns no rows and still joins every collective.  Prints "itilu rank ok" on success."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from tests import itilu_ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=8)
    ap.add_argument("--empty", type=int, default=0)
    args = ap.parse_args()
    import torch.distributed as dist

    dist.init_process_group(backend="gloo")
    rank, size = dist.get_rank(), dist.get_world_size()
    mi = ge.load_binding()
    mi.init()
    mi.init_comm_torch(dist)
    L = itilu_ref.laplace(args.grid, 7)
    N = L.shape[0]
    parts = size - 1 if args.empty else size
    cuts = [mi.row_partition(N, parts, r)[0] for r in range(parts)] + [N] * (size - parts + 1)
    lo, hi = cuts[rank], cuts[rank + 1]
    A = mi.IJMatrix(lo, hi - 1)
    coo = L[lo:hi].tocoo()
    A.set_values_coo(coo.row.astype(np.int64) + lo, coo.col.astype(np.int64), coo.data.astype(np.float64))
    A.assemble()
    block = L[lo:hi, lo:hi].tocsr()
    # type 3, 4 sweeps: the numpy sweeps of this rank's block, bit for bit; norms every sweep, the report all-reduced
    ilu = mi.ILU(iterative_algorithm_type=3, iterative_setup_option=1 | 4 | 8 | 16, iterative_max_iterations=4,
                 print_level=1)
    ilu.setup(A)
    ia, ja, a = ilu.factors()
    assert len(ia) == hi - lo + 1
    if hi > lo:
        P = itilu_ref.Plan(block)
        assert np.array_equal(ia, P.A.indptr) and np.array_equal(ja, P.A.indices)
        assert np.array_equal(a, P.run(4)), np.abs(a - P.run(4)).max()
        assert ilu.iterative_setup_info()[0] == 4
    # type 1 to convergence: the exact ILU(0) of the block
    ilu1 = mi.ILU(iterative_algorithm_type=1, iterative_setup_option=2, iterative_max_iterations=100,
                  iterative_tolerance=0.0)
    ilu1.setup(A)
    a1 = ilu1.factors()[2]
    if hi > lo:
        ex = itilu_ref.exact_ilu0(block)
        assert np.abs(a1 - ex).max() <= 1e-12 * np.abs(ex).max()
    # GMRES with the iterative ILU preconditioner (Jacobi triangular solves)
    f = L @ np.ones(N)
    b = mi.IJVector(lo, hi - 1, f[lo:hi].copy())
    x = mi.IJVector(lo, hi - 1, np.zeros(hi - lo))
    gm = mi.GMRES(tolerance=1e-9, max_iterations=300, kspace=50, print_level=0)
    gm.set_precond(mi.ILU(trisolve=0, iterative_algorithm_type=4, iterative_max_iterations=30))
    gm.setup(A, b, x)
    gm.solve(A, b, x)
    assert gm.final_rel_res < 1e-9 and (hi == lo or np.abs(x.get() - 1.0).max() < 1e-6), gm.final_rel_res
    if not args.empty:
        Ab, bb, xb, _ = mi.build_laplace_system(args.grid + 4, args.grid + 4, args.grid + 4, 7, rank, size)
        amg = mi.BoomerAMG(print_level=0, smooth_type=5, smooth_num_levels=2, ilu_tri_solve=0,
                           iterative_ilu_algorithm_type=3, iterative_ilu_max_iterations=40)
        g2 = mi.GMRES(tolerance=1e-8, max_iterations=100, kspace=50, print_level=0)
        g2.set_precond(amg)
        g2.setup(Ab, bb, xb)
        g2.solve(Ab, bb, xb)
        assert g2.final_rel_res < 1e-8 and np.abs(xb.get() - 1.0).max() < 1e-6
    print(f"itilu rank ok {rank}/{size}: {hi - lo} rows, {gm.num_iterations} GMRES iterations", flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
