"""One rank of the multi-rank Chebyshev check (launched by torch.distributed.run from tests/test_gpu_cheby.py, the
library's own TCP transport, ranks sharing the GPU): the eigenvalue bounds of level 0 against the restatement on the
global operator (Gershgorin also against the one-rank values), one sweep of every order on level 0, and a GMRES solve.
--empty 1: the last rank owns no rows.  Prints "cheby rank ok" on success."""
import argparse
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from tests import cheby_ref  # noqa: E402
from tests.test_cheby_spec import REF_GAP, laplace  # noqa: E402

CG_TOL = max(100.0 * REF_GAP, 1e-13)


def global_level0(amg, dist, size):
    """level 0 of the hierarchy as one scipy matrix in the level's global numbering, and this rank's row range"""
    ia, ja, a, shape = amg.level_csr(0, 0)
    oia, oja, oa, oshape = amg.level_csr(0, 1)
    cm, row_start = amg.level_colmap(0)
    n = shape[0]
    parts = [None] * size
    dist.all_gather_object(parts, (int(row_start), n, ia, ja, a, oia, oja, oa, cm))
    N = sum(p[1] for p in parts)
    rows, cols, vals = [], [], []
    for rs, m, pia, pja, pa, qia, qja, qa, pcm in parts:
        if m == 0:
            continue
        rows.append(rs + np.repeat(np.arange(m), np.diff(pia)))
        cols.append(rs + pja.astype(np.int64))
        vals.append(pa)
        if len(qa):
            rows.append(rs + np.repeat(np.arange(m), np.diff(qia)))
            cols.append(np.asarray(pcm, dtype=np.int64)[qja])
            vals.append(qa)
    G = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N)).tocsr()
    G.sort_indices()
    assert abs(G - G.T).max() == 0.0, "the level's global numbering was not understood"
    return G, int(row_start), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=12)
    ap.add_argument("--seq", type=int, default=-1)
    ap.add_argument("--empty", type=int, default=0)
    args = ap.parse_args()
    import torch  # noqa: F401
    import torch.distributed as dist

    os.environ["MI_HYPRE_LOCALITY_ORDER"] = "0"
    dist.init_process_group(backend="gloo")
    rank, size = dist.get_rank(), dist.get_world_size()
    mi = ge.load_binding()
    mi.init()
    n = args.grid
    L = laplace(n)
    N = L.shape[0]
    # one rank, before the communicator is bound: the Gershgorin bound of level 0
    A1 = mi.matrix_from_scipy(L)
    one = mi.BoomerAMG(print_level=0, relax_type=16, cheby_eig_est=0)
    one.setup(A1)
    gersh_one = one.level_cheby(0)
    one.destroy()
    os.environ["MI_HYPRE_TRANSPORT"] = "tcp"
    os.environ["MI_HYPRE_PORT"] = str(int(os.environ["MASTER_PORT"]) + 100)
    mi.call("HYPRE_MI_CommInitFromEnv")
    parts = size - 1 if args.empty else size
    cuts = [mi.row_partition(N, parts, r)[0] for r in range(parts)] + [N] * (size - parts + 1)
    lo, hi = cuts[rank], cuts[rank + 1]
    A = mi.matrix_from_scipy(L, lo, hi - 1)
    rhs = np.asarray(L @ np.ones(N))
    b = mi.IJVector(lo, hi - 1, rhs[lo:hi].copy())
    x = mi.IJVector(lo, hi - 1, np.zeros(hi - lo))
    kw = dict(print_level=0, relax_type=16)
    if args.seq >= 0:
        kw["seq_threshold"] = args.seq
    rng = np.random.default_rng(11)
    f, u = rng.standard_normal(N), rng.standard_normal(N)
    for est in (0, 10):
        amg = mi.BoomerAMG(cheby_eig_est=est, **kw)
        amg.setup(A)
        G, rs, nloc = global_level0(amg, dist, size)
        assert nloc == hi - lo
        got = amg.level_cheby(0)
        ref = cheby_ref.level_bounds(G, est)
        tol = 1e-14 if est == 0 else CG_TOL
        for key in ("eig_min", "eig_max", "lower", "upper", "theta", "delta"):
            assert abs(got[key] - ref[key]) <= tol * abs(ref["eig_max"]), (est, key, got[key], ref[key])
        if est == 0:
            assert got == gersh_one, (got, gersh_one)
        for order in (1, 2, 3, 4):
            amg.set_cheby(cheby_order=order)
            mine = amg.relax_level(0, 16, 0, f[rs:rs + nloc], u[rs:rs + nloc])
            want = cheby_ref.sweep(G, f, u, got["theta"], got["delta"], order)
            if nloc:
                err = np.abs(mine - want[rs:rs + nloc]).max()
                assert err <= 1e-12 * np.abs(want).max(), (est, order, err)
        amg.set_cheby(cheby_order=2)
        x.fill(0.0)
        gm = mi.GMRES(tolerance=1e-8, max_iterations=100, kspace=10, print_level=0)
        gm.set_precond(amg)
        gm.setup(A, b, x)
        assert gm.solve(A, b, x) == 0
        xs = x.get()
        full = [None] * size
        dist.all_gather_object(full, xs)
        xg = np.concatenate(full)
        res = np.linalg.norm(rhs - L @ xg) / np.linalg.norm(rhs)
        assert res <= 1e-8 and gm.num_iterations <= 100, (res, gm.num_iterations)
    print(f"cheby rank ok {rank}/{size}: {hi - lo} rows, {gm.num_iterations} iterations", flush=True)
    mi.call("HYPRE_MI_CommCheck")
    dist.barrier()
    mi.call("HYPRE_MI_CommFinalize")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
