"""One rank of the multi-rank refusal check of unknown-based systems AMG, launched by torch.distributed.run from
tests/test_systems_amg_spec.py (CPU, gloo, host-only setup): with num_functions > 1 a Setup on more than one rank is
refused by name before anything is built -- with settings that take the distributed setup (PMIS, interp_type 6) and
with settings that take the replicated one (interp_type 17) -- and num_functions 1 still sets up.  Prints
"systems rank ok" on success."""
import os
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
    for interp in (6, 17):
        amg = mi.BoomerAMG(print_level=0, interp_type=interp, num_functions=2)
        try:
            mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
        except mi.HypreError as e:
            want = "num_functions 2 is not implemented on more than one rank (%d ranks)" % size
            assert want in str(e), str(e)
            mi.call("HYPRE_ClearAllErrors")
        else:
            raise AssertionError("num_functions 2 on %d ranks was not refused (interp_type %d)" % (size, interp))
        ok = mi.BoomerAMG(print_level=0, interp_type=interp, num_functions=1)
        mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", ok.h, A.par)
        assert ok.num_levels >= 2
    print(f"systems rank ok {rank}/{size}", flush=True)
    dist.barrier()
    mi.call("HYPRE_MI_CommFinalize")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
