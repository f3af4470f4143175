"""One rank of the multi-rank check of the matrix-matrix extended interpolation (interp_type 16 / 17), launched by
torch.distributed.run from tests/test_mm_interp_spec.py (CPU, gloo, host-only setup).

Hierarchies with interp_type 16 / 17 are built by the replicated setup on N > 1 ranks: every rank builds the global
hierarchy and keeps its slices.  Before the communicator exists every rank therefore builds the single-rank hierarchy
of the global operator (the reference), then the N-rank one, and compares every level's operator, C/F marker and
interpolation, entry for entry, through the natural numbering.  Prints "mm_interp rank ok" on success."""
import argparse
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from tests.agg2s_dist_worker import csr, identical, single_rank_reference  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=12)
    ap.add_argument("--interp", type=int, default=17)
    ap.add_argument("--seq", type=int, default=0, help="redundant-level threshold; 0 = none")
    args = ap.parse_args()
    import torch  # noqa: F401
    import torch.distributed as dist

    os.environ["MI_HYPRE_LOCALITY_ORDER"] = "0"
    dist.init_process_group(backend="gloo")
    rank, size = dist.get_rank(), dist.get_world_size()
    mi = ge.load_binding()
    n = args.grid
    kw = dict(print_level=0, interp_type=args.interp, true_pmax_elmts=4, seq_threshold=args.seq)

    # ---- the reference: one rank, before the communicator is bound
    A1, _ = mi.build_laplace_system_host(n, n, n, 7, 0, 1)
    ref_amg = mi.BoomerAMG(**kw)
    mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", ref_amg.h, A1.par)
    ref = single_rank_reference(ref_amg)
    mi.init_comm_torch(dist)

    def counter(name):
        v = mi.C.c_longlong()
        mi.call("HYPRE_MI_GetCounter", name.encode(), mi.C.byref(v))
        return v.value

    amg = mi.BoomerAMG(**kw)
    A, _ = mi.build_laplace_system_host(n, n, n, 7, rank, size)
    mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
    assert counter("setup_distributed") == 0, "interp_type 16 / 17 must take the replicated setup"
    nl = amg.num_levels
    assert nl == ref_amg.num_levels >= 3, (nl, ref_amg.num_levels)

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
        r, c, v = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)], [np.zeros(0)]
        for M, cols in ((D, np.arange(D.shape[1], dtype=np.int64) + col_start), (O, cm.astype(np.int64))):
            M = M.tocoo()
            if M.nnz:
                r.append(M.row), c.append(colmap_to_natural(cols[M.col])), v.append(M.data)
        return sp.csr_matrix((np.concatenate(v), (np.concatenate(r), np.concatenate(c))), shape=(D.shape[0], ncols_global))

    for l in range(nl):
        table, row_start, mine_nat = natural_of_new(l)
        Nl = ref[l]["A"].shape[0]
        assert len(table) == Nl and np.array_equal(np.sort(table), np.arange(Nl)), (l, rank)
        assert identical(my_rows(l, 0, 1, row_start, Nl, lambda c: table[c]), ref[l]["A"][mine_nat]), (l, rank)
        if l == nl - 1:
            continue
        assert np.array_equal(amg.level_cf(l), ref[l]["cf"][mine_nat]), (l, rank)
        tablec, row_start_c, _ = natural_of_new(l + 1)
        Pm = my_rows(l, 2, 4, row_start_c, ref[l]["P"].shape[1], lambda c: tablec[c])
        assert identical(Pm, ref[l]["P"][mine_nat]), (l, rank)
    print(f"mm_interp rank ok {rank}/{size}: {nl} levels equal the single-rank hierarchy", flush=True)
    dist.barrier()
    mi.call("HYPRE_MI_CommFinalize")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
