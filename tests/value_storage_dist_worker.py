"""Value storage of BoomerAMG on two ranks that share the GPU (torchrun, the library's own TCP transport): per rank
mode 1 and mode 2 give the same bits, the operators that are narrowed are the ones a single rank narrows (kinds per
level), the solve converges, and an operator whose values do not fit on one rank keeps fp64 on both.
tests/test_gpu_value_storage.py counts the "value storage rank ok" lines."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def kinds_of(amg):
    """per level: the kinds of A, P and R (diag blocks; a value dictionary counts as the mode it was built in)"""
    out = []
    for l in range(amg.num_levels):
        ws = (0,) if l == amg.num_levels - 1 else (0, 2, 3)
        out.append(tuple(amg.level_value_storage(l, w)[0] for w in ws))
    return out


def run(mi, n, rank, size, mode):
    A, b, x, _ = mi.build_laplace_system(n, n, n, 7, rank, size)
    amg = mi.BoomerAMG(print_level=0, mi_value_storage=mode)
    gm = mi.GMRES(tolerance=1e-9, max_iterations=100, kspace=50, print_level=0)
    gm.set_precond(amg)
    gm.setup(A, b, x)
    assert gm.solve(A, b, x) == 0
    xs = x.get()
    assert gm.final_rel_res < 1e-9 and np.abs(xs - 1.0).max() < 1e-6, (mode, gm.final_rel_res)
    return dict(iters=gm.num_iterations, hist=gm.residual_history(), x=xs, kinds=kinds_of(amg), levels=amg.num_levels)


FLT_MIN, FLT_MAX = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)


def fits(a):
    m = np.abs(a[np.isfinite(a) & (a != 0.0)])
    return not (np.any(m > FLT_MAX) or np.any(m < FLT_MIN))


def badly_scaled(n):
    """two uncoupled 7-point operators on n x n x n/2 grids, the second times 2^-132: rank 0's rows hold ordinary
    values on every level, rank 1's rows values below FLT_MIN"""
    import scipy.sparse as sp
    lap1 = lambda k: sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(k, k))
    h, I, Ih = n // 2, sp.identity(n), sp.identity(n // 2)
    B = sp.kron(sp.kron(lap1(h), I), I) + sp.kron(sp.kron(Ih, lap1(n)), I) + sp.kron(sp.kron(Ih, I), lap1(n))
    return sp.csr_matrix(sp.block_diag([B, 2.0 ** -132 * B]))


def run_fallback(mi, M, rank, size, mode):
    """setup and one V-cycle with every level distributed (seq_threshold 0)"""
    lo, hi = mi.row_partition(M.shape[0], size, rank)
    A = mi.matrix_from_scipy(M, lo, hi)
    amg = mi.BoomerAMG(print_level=0, mi_value_storage=mode, seq_threshold=0)
    amg.setup(A)
    b = mi.IJVector(lo, hi, np.cos(np.arange(lo, hi + 1, dtype=np.float64)))
    x = mi.IJVector(lo, hi, np.zeros(hi - lo + 1))
    amg.solve(A, b, x)
    blocks = np.concatenate([amg.level_csr(1, 0)[2], amg.level_csr(1, 1)[2]])
    return dict(kinds=kinds_of(amg), x=x.get(), levels=amg.num_levels, a1_fits_here=fits(blocks))


def fallback_on_two_ranks(mi, rank, size):
    """An operator that one rank alone would narrow keeps fp64 on every rank when another rank's part does not fit."""
    M = badly_scaled(12)
    r = {m: run_fallback(mi, M, rank, size, m) for m in (0, 1, 2)}
    assert r[0]["levels"] > 2 and r[1]["levels"] == r[2]["levels"] == r[0]["levels"]
    assert r[0]["a1_fits_here"] == (rank == 0), (rank, r[0]["a1_fits_here"])  # the case is what it is meant to be
    for m in (1, 2):
        assert all(row[0] == 0 for row in r[m]["kinds"][1:]), (rank, m, r[m]["kinds"])  # A_l, l >= 1: kept, everywhere
        assert all(k in (m, 8) for row in r[m]["kinds"][1:] for k in row[1:]), (rank, m, r[m]["kinds"])  # P_l, R_l: narrowed
    assert np.array_equal(r[1]["x"].view(np.int64), r[2]["x"].view(np.int64))
    assert np.all(np.isfinite(r[1]["x"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=20)
    args = ap.parse_args()
    import torch  # noqa: F401
    import torch.distributed as dist

    os.environ["MI_HYPRE_LOCALITY_ORDER"] = "0"
    dist.init_process_group(backend="gloo")
    rank, size = dist.get_rank(), dist.get_world_size()
    mi = ge.load_binding()
    mi.init()
    n = args.grid
    one = {m: run(mi, n, 0, 1, m) for m in (0, 1, 2)}  # one rank, before the communicator is bound
    os.environ["MI_HYPRE_TRANSPORT"] = "tcp"
    os.environ["MI_HYPRE_PORT"] = str(int(os.environ["MASTER_PORT"]) + 100)
    mi.call("HYPRE_MI_CommInitFromEnv")
    two = {m: run(mi, n, rank, size, m) for m in (0, 1, 2)}
    for r in (one, two):
        assert r[1]["iters"] == r[2]["iters"] and np.array_equal(r[1]["hist"].view(np.int64), r[2]["hist"].view(np.int64))
        assert np.array_equal(r[1]["x"].view(np.int64), r[2]["x"].view(np.int64))
        assert r[1]["iters"] <= r[0]["iters"] + 1, (r[1]["iters"], r[0]["iters"])
    assert two[1]["levels"] == one[1]["levels"]
    for m in (1, 2):
        # a dictionary (kind 8) depends on the block's size: compare "narrowed or not"
        norm = lambda ks: [tuple(m if k == 8 else k for k in row) for row in ks]
        assert norm(two[m]["kinds"]) == norm(one[m]["kinds"]), (m, two[m]["kinds"], one[m]["kinds"])
        assert all(k == m for row in norm(two[m]["kinds"])[1:] for k in row), two[m]["kinds"]
        assert all(k in (0, 8) for k in two[m]["kinds"][0])
    fallback_on_two_ranks(mi, rank, size)
    print(f"value storage rank ok {rank}/{size}: {two[1]['iters']} iterations in modes 1 and 2, {two[0]['iters']} in mode 0",
          flush=True)
    mi.call("HYPRE_MI_CommCheck")
    dist.barrier()
    mi.call("HYPRE_MI_CommFinalize")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
