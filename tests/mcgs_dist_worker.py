"""One rank of the multi-rank check of relax types 40 / 41 / 42, launched by torch.distributed.run from
tests/test_mcgs_spec.py (CPU, gloo): the multicolour Gauss-Seidel smoother is refused on more than one rank, in any slot,
with a message that names the rank count -- on every rank, before anything collective starts.  Prints "mcgs rank ok"."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def main():
    import torch  # noqa: F401
    import torch.distributed as dist

    os.environ["MI_HYPRE_LOCALITY_ORDER"] = "0"
    dist.init_process_group(backend="gloo")
    rank, size = dist.get_rank(), dist.get_world_size()
    mi = ge.load_binding()
    mi.init_comm_torch(dist)
    A, _ = mi.build_laplace_system_host(8, 8, 8, 7, rank, size)
    for kw in (dict(relax_type=40), dict(down_relax_type=8, up_relax_type=41, coarse_relax_type=9),
               dict(down_relax_type=8, up_relax_type=8, coarse_relax_type=42)):
        t = max(v for v in kw.values())
        amg = mi.BoomerAMG(print_level=0, **kw)
        try:
            mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
            raise AssertionError("relax type %d was accepted on %d ranks" % (t, size))
        except mi.HypreError as e:
            assert re.search(r"relax_type %d \(multicolour Gauss-Seidel\) is not implemented on more than one rank \(%d ranks\)"
                             % (t, size), str(e)), str(e)
        mi.call("HYPRE_ClearAllErrors")
    amg = mi.BoomerAMG(print_level=0)  # (the default smoother still builds)
    mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
    assert amg.num_levels >= 2
    print(f"mcgs rank ok {rank}/{size}", flush=True)
    dist.barrier()
    mi.call("HYPRE_MI_CommFinalize")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
