"""Update rounds of an IJ matrix on ranks that share the GPU (direct children, the library's own TCP transport): the
7-point 12^3 operator by slabs of rows, so every rank that owns rows has a halo block.  argv[1] == "empty": the last
rank's rows go to the one before it and it owns none.  Rounds, all through device pointers:
  1  every rank sets new values of all its entries, diag and halo block, shuffled;
  2  rank 0 submits nothing (it opens its round with Initialize: Assemble is collective), the others add;
  3  ONE rank submits a halo entry that is not in the pattern: Assemble fails on every rank, no rank's values change.
After each round the snapshot (blocks, column map, a distributed product) equals that of a fresh host assembly of all
batches so far.  tests/test_gpu_ij_update.py counts the "ij update rank ok" lines."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from tests import ij_cases as cases  # noqa: E402

N = 12


def fresh(mi, lo, hi, batches):
    A = cases.new_matrix(mi, lo, hi)
    cases.stage(mi, A, batches, False)
    A.assemble()
    return cases.snapshot(mi, A)


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
    if len(sys.argv) > 1 and sys.argv[1] == "empty":  # a rank without rows takes part
        if rank == size - 1:
            lo, hi = total, total - 1
        elif rank == size - 2:
            hi = total - 1
    rng = np.random.default_rng(300 + rank)
    own = hi >= lo
    r, c, v = cases.laplace_triples(mi, N, 7, lo, hi) if own else (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0))
    first = [(r, c, v, False)] if own else []
    A = cases.new_matrix(mi, lo, hi)
    cases.stage(mi, A, first, True)
    A.assemble()
    assert own == (len(mi.parcsr_colmap(A)) > 0)
    halo = (c < lo) | (c > hi)

    def round_(batches, expect_failure=False):
        d0 = mi.counter("ij_device_value_updates")
        A.initialize()
        cases.stage(mi, A, batches, True)
        if expect_failure:
            try:
                A.assemble()
            except mi.HypreError as e:
                mi.call("HYPRE_ClearAllErrors")
                return str(e)
            raise AssertionError("the refused round was applied")
        A.assemble()
        assert mi.counter("ij_device_value_updates") - d0 == (1 if batches else 0)
        return None

    # 1: diag and halo values change on every rank
    p = rng.permutation(len(v))
    b1 = [(r[p].copy(), c[p].copy(), (1.5 * v + rng.standard_normal(len(v)))[p], False)] if own else []
    round_(b1)
    s1 = cases.snapshot(mi, A)
    assert cases.same(s1, fresh(mi, lo, hi, first + b1))
    # 2: rank 0 contributes nothing
    b2 = [(r[halo].copy(), c[halo].copy(), rng.standard_normal(int(halo.sum())), True),
          (r[:50].copy(), c[:50].copy(), np.full(50, 0.125), True)] if own and rank != 0 else []
    round_(b2)
    s2 = cases.snapshot(mi, A)
    assert cases.same(s2, fresh(mi, lo, hi, first + b1 + b2))
    if rank == 0 and own:
        assert np.array_equal(s2["a0"], s1["a0"]) and np.array_equal(s2["a1"], s1["a1"])
    # 3: rank 1 submits a halo entry outside its pattern (column 0 is far from its first row), after good ones
    stamp = mi.assembly_stamp(A)
    b3 = [(r.copy(), c.copy(), 2.0 * v, False)] if own else []
    if rank == 1:
        b3.append((np.array([lo], dtype=np.int64), np.array([0], dtype=np.int64), np.array([1.0]), True))
    msg = round_(b3, expect_failure=True)
    assert ("row %d, column 0)" % lo in msg) if rank == 1 else ("another rank" in msg), msg
    assert mi.assembly_stamp(A) == stamp
    assert cases.same(cases.snapshot(mi, A), s2)
    # and a good round afterwards
    round_(b3[:1])
    assert cases.same(cases.snapshot(mi, A), fresh(mi, lo, hi, first + b1 + b2 + b3[:1]))
    print(f"ij update rank ok {rank}/{size}", flush=True)
    mi.call("HYPRE_MI_CommCheck")
    dist.barrier()
    mi.call("HYPRE_MI_CommFinalize")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
