"""One rank of the multi-rank checks of the two-stage extended interpolation (agg_interp_type 5), launched by
torch.distributed.run from tests/test_agg2s_spec.py (--mode host, CPU, gloo) and tests/test_gpu_agg2s.py (--mode solve,
ranks sharing the GPU, the library's TCP transport).

Hierarchies with agg_interp_type 5 on aggressive levels are built by the replicated setup on N > 1 ranks: every rank
builds the global hierarchy and keeps its slices.  Before the communicator exists every rank therefore builds the
single-rank hierarchy of the global operator (the reference), then the N-rank one, and compares
  host:  every level's operator, C/F marker and interpolation, entry for entry, through the natural numbering;
  solve: the GMRES + AMG iteration count and the solution x* = 1.
Prints "agg2s rank ok" on success."""
import argparse
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def csr(amg, level, which):
    ia, ja, a, shape = amg.level_csr(level, which)
    return sp.csr_matrix((a, ja, ia), shape=shape)


def identical(X, Y):
    X, Y = sp.csr_matrix(X), sp.csr_matrix(Y)
    if X.shape != Y.shape or X.nnz != Y.nnz:
        return False
    D = abs(X - Y)
    return D.nnz == 0 or D.max() == 0.0


def single_rank_reference(amg):
    """per level: A, C/F marker and P in the level's natural numbering (level_csr reports C-first renumbered copies)"""
    out = []
    nl = amg.num_levels
    perms = [amg.level_perm(l).astype(np.int64) for l in range(nl)]
    for l in range(nl):
        n = len(perms[l])
        Q = sp.csr_matrix((np.ones(n), (perms[l], np.arange(n))), shape=(n, n))  # natural <- reported
        lev = dict(A=(Q @ csr(amg, l, 0) @ Q.T).tocsr(), A_reported=csr(amg, l, 0), perm=perms[l])
        if l < nl - 1:
            nc = len(perms[l + 1])
            Qc = sp.csr_matrix((np.ones(nc), (perms[l + 1], np.arange(nc))), shape=(nc, nc))
            cf = np.empty(n, dtype=np.int32)
            cf[perms[l]] = amg.level_cf(l)
            lev.update(P=(Q @ csr(amg, l, 2) @ Qc.T).tocsr(), P_reported=csr(amg, l, 2), cf=cf, cf_reported=amg.level_cf(l))
        out.append(lev)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="host")
    ap.add_argument("--grid", type=int, default=12)
    ap.add_argument("--seq", type=int, default=-1, help="redundant-level threshold; -1 = library default, 0 = none")
    ap.add_argument("--agg", type=int, default=1)
    ap.add_argument("--transport", default="callbacks", help="callbacks (gloo) | tcp (the library's own TCP mesh)")
    args = ap.parse_args()
    import torch  # noqa: F401
    import torch.distributed as dist

    os.environ["MI_HYPRE_LOCALITY_ORDER"] = "0"
    dist.init_process_group(backend="gloo")
    rank, size = dist.get_rank(), dist.get_world_size()
    mi = ge.load_binding()
    n = args.grid
    N = n ** 3
    kw = dict(print_level=0, agg_num_levels=args.agg, agg_interp_type=5, agg_pmax_elmts=4)
    if args.seq >= 0:
        kw["seq_threshold"] = args.seq

    # ---- the reference: one rank, before the communicator is bound
    if args.mode == "host":
        A1, _ = mi.build_laplace_system_host(n, n, n, 7, 0, 1)
        ref_amg = mi.BoomerAMG(**kw)
        mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", ref_amg.h, A1.par)
        ref = single_rank_reference(ref_amg)
        ref_levels = ref_amg.num_levels
    else:
        mi.init()
        A1, b1, x1, _ = mi.build_laplace_system(n, n, n, 7)
        ref_amg = mi.BoomerAMG(**kw)
        g1 = mi.GMRES(tolerance=1e-8, max_iterations=100, kspace=50, print_level=0)
        g1.set_precond(ref_amg)
        g1.setup(A1, b1, x1)
        assert g1.solve(A1, b1, x1) == 0
        ref_iters, ref_levels = g1.num_iterations, ref_amg.num_levels
        assert np.abs(x1.get() - 1.0).max() < 1e-6

    if args.transport == "tcp":
        os.environ["MI_HYPRE_TRANSPORT"] = "tcp"
        os.environ["MI_HYPRE_PORT"] = str(int(os.environ["MASTER_PORT"]) + 100)
        mi.call("HYPRE_MI_CommInitFromEnv")
    else:
        mi.init_comm_torch(dist)

    def counter(name):
        v = mi.C.c_longlong()
        mi.call("HYPRE_MI_GetCounter", name.encode(), mi.C.byref(v))
        return v.value

    amg = mi.BoomerAMG(**kw)
    if args.mode == "solve":
        A, b, x, _ = mi.build_laplace_system(n, n, n, 7, rank, size)
        gm = mi.GMRES(tolerance=1e-8, max_iterations=100, kspace=50, print_level=0)
        gm.set_precond(amg)
        gm.setup(A, b, x)
        assert gm.solve(A, b, x) == 0
        assert counter("setup_distributed") == 0, "type 5 on aggressive levels must take the replicated setup"
        assert amg.num_levels == ref_levels
        assert gm.final_rel_res < 1e-8 and np.abs(x.get() - 1.0).max() < 1e-6
        assert gm.num_iterations == ref_iters, (gm.num_iterations, ref_iters)
        print(f"agg2s rank ok {rank}/{size}: {gm.num_iterations} iterations on {size} ranks and on one", flush=True)
        mi.call("HYPRE_MI_CommCheck")
        dist.barrier()
        mi.call("HYPRE_MI_CommFinalize")
        dist.destroy_process_group()
        return

    A, _ = mi.build_laplace_system_host(n, n, n, 7, rank, size)
    mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
    assert counter("setup_distributed") == 0, "type 5 on aggressive levels must take the replicated setup"
    assert amg.num_levels == ref_levels, (amg.num_levels, ref_levels)
    nl = amg.num_levels
    redundant = lambda l: size > 1 and l >= 1 and args.seq != 0 and ref[l]["A"].shape[0] <= (args.seq if args.seq > 0 else 200000)

    def gather(obj):
        parts = [None] * size
        dist.all_gather_object(parts, obj)
        return parts

    def natural_of_new(l):
        """global natural id of every global id of distributed level l, this rank's first row, its natural rows"""
        perm = amg.level_perm(l).astype(np.int64)
        _, row_start = amg.level_colmap(l)
        parts = gather((int(row_start), perm))
        table = np.concatenate([s + p for s, p in parts])  # (rank order = ascending first rows)
        return table, int(row_start), row_start + perm

    def my_rows(l, diag, offd, col_start, ncols_global, colmap_to_natural):
        D, O = csr(amg, l, diag), csr(amg, l, offd)
        cm = amg.level_offd_colmap(l, offd)
        rows = []
        for M, cols in ((D, np.arange(D.shape[1], dtype=np.int64) + col_start), (O, cm.astype(np.int64))):
            M = M.tocoo()
            if M.nnz:
                rows.append((M.row, colmap_to_natural(cols[M.col]), M.data))
        r = np.concatenate([t[0] for t in rows]) if rows else np.zeros(0, dtype=np.int64)
        c = np.concatenate([t[1] for t in rows]) if rows else np.zeros(0, dtype=np.int64)
        v = np.concatenate([t[2] for t in rows]) if rows else np.zeros(0)
        return sp.csr_matrix((v, (r, c)), shape=(D.shape[0], ncols_global))

    for l in range(nl):
        last = l == nl - 1
        if redundant(l):
            # every rank holds the whole level, in the single-rank C-first ordering
            assert identical(csr(amg, l, 0), ref[l]["A_reported"]), (l, rank)
            if not last:
                assert np.array_equal(amg.level_cf(l), ref[l]["cf_reported"]), (l, rank)
                assert np.array_equal(amg.level_perm(l), ref[l]["perm"]), (l, rank)
                assert identical(csr(amg, l, 2), ref[l]["P_reported"]), (l, rank)
            continue
        table, row_start, mine_nat = natural_of_new(l)
        Nl = ref[l]["A"].shape[0]
        assert len(table) == Nl and np.array_equal(np.sort(table), np.arange(Nl)), (l, rank)
        Am = my_rows(l, 0, 1, row_start, Nl, lambda c: table[c])
        assert identical(Am, ref[l]["A"][mine_nat]), (l, rank)
        if last:
            continue
        cf = amg.level_cf(l)
        assert np.array_equal(cf, ref[l]["cf"][mine_nat]), (l, rank)
        Nc = ref[l]["P"].shape[1]
        if redundant(l + 1):
            # the next level is numbered naturally there: slices = the owners of the C points
            counts = gather(int((cf == 1).sum()))
            col_start = int(sum(counts[:rank]))
            Pm = my_rows(l, 2, 4, col_start, Nc, lambda c: c)
        else:
            tablec, row_start_c, _ = natural_of_new(l + 1)
            Pm = my_rows(l, 2, 4, row_start_c, Nc, lambda c: tablec[c])
        assert identical(Pm, ref[l]["P"][mine_nat]), (l, rank)
    print(f"agg2s rank ok {rank}/{size}: {nl} levels equal the single-rank hierarchy", flush=True)
    dist.barrier()
    mi.call("HYPRE_MI_CommFinalize")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
