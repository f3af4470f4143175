"""One rank of the multi-rank FSAI check (launched by torch.distributed.run from tests/test_gpu_fsai.py): BoomerAMG with
the FSAI smoother on ranks sharing the GPU.  Every rank's G must equal the numpy FSAI of its own diagonal block, omega
must be the same on every rank and equal the numpy power iteration with all-reduced inner products, and GMRES must
converge.  Prints "fsai rank ok" on success."""
import argparse
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from tests import fsai_ref  # noqa: E402


def laplace(n):
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n))
    I = sp.identity(n)
    return (sp.kron(sp.kron(I, I), T) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(T, I), I)).tocsr()


def empty_rank_check(mi, dist, torch, n, rank, size):
    """The rows split over ranks 0 .. size-2, none on the last one: HYPRE_FSAISetup and 30 Richardson steps of
    HYPRE_FSAISolve on every rank, against the numpy block-Jacobi FSAI of the same partition."""
    L = laplace(n)
    N = L.shape[0]
    cuts = [mi.row_partition(N, size - 1, r)[0] for r in range(size - 1)] + [N, N]
    lo, hi = cuts[rank], cuts[rank + 1]
    A = mi.IJMatrix(lo, hi - 1)
    coo = L[lo:hi].tocoo()
    A.set_values_coo(coo.row.astype(np.int64) + lo, coo.col.astype(np.int64), coo.data.astype(np.float64))
    A.assemble()
    rng = np.random.default_rng(7)
    f = rng.standard_normal(N)
    b = mi.IJVector(lo, hi - 1, f[lo:hi].copy())
    x = mi.IJVector(lo, hi - 1, np.zeros(hi - lo))
    fs = mi.FSAI(max_iterations=30, tolerance=0.0, zero_guess=1)
    fs.setup(A)
    fs.solve(A, b, x)
    # numpy: block-diagonal G over the ranks' diagonal blocks, omega by the global power iteration on G B G^T
    blocks = [fsai_ref.factor(L[cuts[r]:cuts[r + 1], cuts[r]:cuts[r + 1]], 0.01, 1) for r in range(size - 1)]
    G = sp.block_diag(blocks).tocsr()
    Bd = sp.block_diag([L[cuts[r]:cuts[r + 1], cuts[r]:cuts[r + 1]] for r in range(size - 1)]).tocsr()
    om = fsai_ref.omega(G, Bd, 5)
    xr = np.zeros(N)
    for it in range(30):
        xr = fsai_ref.smooth(G, om, L, f, None if it == 0 else xr)
    mine = x.get()
    assert mine.shape == (hi - lo,)
    if hi > lo:
        ref = xr[lo:hi]
        assert np.abs(mine - ref).max() <= 1e-10 * np.abs(ref).max(), np.abs(mine - ref).max()
    print(f"fsai rank ok {rank}/{size}: {hi - lo} rows", flush=True)
    dist.barrier()
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=12)
    ap.add_argument("--seq", type=int, default=-1)
    ap.add_argument("--empty", type=int, default=0, help="1: the last rank owns no rows (standalone FSAI on that partition)")
    args = ap.parse_args()
    import torch
    import torch.distributed as dist

    dist.init_process_group(backend="gloo")
    rank, size = dist.get_rank(), dist.get_world_size()
    mi = ge.load_binding()
    mi.init()
    mi.init_comm_torch(dist)
    n = args.grid
    if args.empty:
        empty_rank_check(mi, dist, torch, n, rank, size)
        return
    A, b, x, rhs = mi.build_laplace_system(n, n, n, 7, rank, size)
    kw = dict(print_level=0, smooth_type=4, smooth_num_levels=50)
    if args.seq >= 0:
        kw["seq_threshold"] = args.seq
    amg = mi.BoomerAMG(**kw)
    gm = mi.GMRES(tolerance=1e-8, max_iterations=100, kspace=50, print_level=0)
    gm.set_precond(amg)
    gm.setup(A, b, x)
    assert gm.solve(A, b, x) == 0
    assert gm.final_rel_res < 1e-8 and np.abs(x.get() - 1.0).max() < 1e-6

    def allsum(v):
        t = torch.tensor([float(v)], dtype=torch.float64)
        dist.all_reduce(t)
        return float(t[0])

    got = amg.level_fsai(0)
    assert got is not None
    ia, ja, a, om = got
    bia, bja, ba, shape = amg.level_csr(0, 0)
    _, row_start = amg.level_colmap(0)
    B = sp.csr_matrix((ba, bja, bia), shape=shape)
    G = sp.csr_matrix((a, ja, ia), shape=shape)
    Gr = fsai_ref.factor(B, 0.01, 1)
    assert np.array_equal(G.indptr, Gr.indptr) and np.array_equal(G.indices, Gr.indices)
    assert np.abs(G.data - Gr.data).max() <= 1e-12 * np.abs(Gr.data).max()
    om_ref = fsai_ref.omega(G, B, 5, gid0=row_start, dot=lambda u, v: allsum(u @ v))
    assert abs(om - om_ref) <= 1e-12 * om_ref, (om, om_ref)
    oms = [None] * size
    dist.all_gather_object(oms, om)
    assert all(o == oms[0] for o in oms), oms
    print(f"fsai rank ok {rank}/{size}: {gm.num_iterations} iterations, omega {om:.12g}", flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
