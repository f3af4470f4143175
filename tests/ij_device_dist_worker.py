"""Device IJ assembly on ranks that share the GPU (direct children, the library's own TCP transport): every rank
assembles its block rows of the shuffled 7-point 12^3 operator with duplicates from device arrays and from numpy
arrays; diag, offd, column map, halo plan and a product are the same bit for bit -- also on a partition that leaves a
rank without rows -- and the distributed solve takes the same iterations.
tests/test_gpu_ij_device_assembly.py counts the "ij device assembly rank ok" lines."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from tests import ij_cases as cases  # noqa: E402

N = 12


def my_batches(mi, lo, hi, seed):
    """this rank's rows, shuffled; a tenth of the entries again in an Add batch"""
    if hi < lo:
        return []
    r, c, v = cases.laplace_triples(mi, N, 7, lo, hi)
    rng = np.random.default_rng(seed)
    p = rng.permutation(len(v))
    r, c, v = r[p], c[p], v[p]
    k = max(1, len(v) // 10)
    return [(r.copy(), c.copy(), v.copy(), False), (r[:k].copy(), c[:k].copy(), 0.5 * v[:k], True)]


def assemble(mi, lo, hi, batches, device):
    A = cases.new_matrix(mi, lo, hi)
    before = mi.counter("ij_device_assemblies")
    cases.stage(mi, A, batches, device)
    A.assemble()
    assert mi.counter("ij_device_assemblies") - before == (1 if device and batches else 0)
    return A


def compare(mi, lo, hi, batches):
    Ad, Ah = assemble(mi, lo, hi, batches, True), assemble(mi, lo, hi, batches, False)
    assert cases.same(cases.snapshot(mi, Ad), cases.snapshot(mi, Ah))
    pd, ph = mi.halo_plan(Ad), mi.halo_plan(Ah)
    for k in ph:
        assert np.array_equal(pd[k], ph[k]), k
    return Ad, Ah


def solve(mi, A, lo, hi):
    n = hi - lo + 1
    b = mi.IJVector(lo, hi, np.cos(np.arange(lo, hi + 1, dtype=np.float64)))
    x = mi.IJVector(lo, hi, np.zeros(n))
    amg = mi.BoomerAMG(print_level=0)
    gm = mi.GMRES(tolerance=1e-8, max_iterations=60, kspace=50, print_level=0)
    gm.set_precond(amg)
    gm.setup(A, b, x)
    assert gm.solve(A, b, x) == 0
    return gm.num_iterations, gm.residual_history().view(np.int64)


def main():
    import torch  # noqa: F401
    import torch.distributed as dist

    os.environ["MI_HYPRE_LOCALITY_ORDER"] = "0"
    dist.init_process_group(backend="gloo")
    rank, size = dist.get_rank(), dist.get_world_size()
    mi = ge.load_binding()
    mi.init()
    os.environ["MI_HYPRE_TRANSPORT"] = "tcp"
    os.environ["MI_HYPRE_PORT"] = str(int(os.environ["MASTER_PORT"]) + 100)
    mi.call("HYPRE_MI_CommInitFromEnv")
    total = N ** 3
    lo, hi = mi.row_partition(total, size, rank)
    Ad, Ah = compare(mi, lo, hi, my_batches(mi, lo, hi, 100 + rank))
    assert len(mi.parcsr_colmap(Ad)) > 0
    it_d, hist_d = solve(mi, Ad, lo, hi)
    it_h, hist_h = solve(mi, Ah, lo, hi)
    assert it_d == it_h and np.array_equal(hist_d, hist_h), (it_d, it_h)
    # the same with the last rank's rows given to the one before it: a rank without rows takes part
    if rank == size - 1:
        lo2, hi2 = total, total - 1
    elif rank == size - 2:
        lo2, hi2 = lo, total - 1
    else:
        lo2, hi2 = lo, hi
    compare(mi, lo2, hi2, my_batches(mi, lo2, hi2, 200 + rank))
    print(f"ij device assembly rank ok {rank}/{size}: {it_d} iterations", flush=True)
    mi.call("HYPRE_MI_CommCheck")
    dist.barrier()
    mi.call("HYPRE_MI_CommFinalize")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
