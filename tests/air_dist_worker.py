"""One rank of the multi-rank check of restriction 1 and interp_type 100, launched by torch.distributed.run from
tests/test_air_spec.py (CPU, gloo, host-only setup): the approximate ideal restriction is refused on more than one rank
with a message that says so -- on every rank, before anything collective starts -- and one-point interpolation builds
(replicated setup) with R = P^T.  Prints "air rank ok" on success."""
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
    amg = mi.BoomerAMG(print_level=0, restriction=1)
    try:
        mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
        raise AssertionError("restriction 1 was accepted on %d ranks" % size)
    except mi.HypreError as e:
        assert re.search(r"restriction 1 \(approximate ideal restriction\) is not implemented on more than one rank \(%d ranks\)" % size,
                         str(e)), str(e)
    mi.call("HYPRE_ClearAllErrors")
    amg = mi.BoomerAMG(print_level=0, interp_type=100)
    mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
    assert amg.num_levels >= 2 and amg.restriction_info(0)["kind"] == 0
    print(f"air rank ok {rank}/{size}", flush=True)
    dist.barrier()
    mi.call("HYPRE_MI_CommFinalize")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
