"""One rank of the multi-rank check of FSAI with the adaptive pattern (launched by torch.distributed.run from
tests/test_gpu_fsai_adaptive.py): BoomerAMG with the FSAI smoother, algo type 4, on ranks sharing the GPU.  Every rank's
G must equal the numpy restatement on its own diagonal block (block Jacobi), omega must be the same on every rank and
equal the numpy power iteration with all-reduced inner products, and GMRES must converge.  Prints "fsai adaptive rank
ok" on success."""
import argparse
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from tests import fsai_adaptive_cases as fc  # noqa: E402
from tests import fsai_adaptive_ref as ref  # noqa: E402
from tests import fsai_ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=10)
    args = ap.parse_args()
    import torch
    import torch.distributed as dist

    dist.init_process_group(backend="gloo")
    rank, size = dist.get_rank(), dist.get_world_size()
    mi = ge.load_binding()
    mi.init()
    mi.init_comm_torch(dist)
    n = args.grid
    A, b, x, rhs = mi.build_laplace_system(n, n, n, 7, rank, size)
    amg = mi.BoomerAMG(print_level=0, smooth_type=4, smooth_num_levels=50, fsai_algo_type=4, fsai_max_steps=4,
                       fsai_max_step_size=3, fsai_kap_tolerance=1e-2)
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
    Gr, rinfo = ref.factor(B, 4, 3, 1e-2)
    fc.same_G(G, Gr)
    fc.same_counts(amg.level_fsai_info(0), rinfo)
    om_ref = fsai_ref.omega(G, B, 5, gid0=row_start, dot=lambda u, v: allsum(u @ v))
    assert abs(om - om_ref) <= 1e-12 * om_ref, (om, om_ref)
    oms = [None] * size
    dist.all_gather_object(oms, om)
    assert all(o == oms[0] for o in oms), oms
    print(f"fsai adaptive rank ok {rank}/{size}: {gm.num_iterations} iterations, omega {om:.12g}", flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
