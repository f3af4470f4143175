"""CPU: the specification of an update round of an assembled IJ matrix (HYPRE_IJMatrixSetValues / AddToValues /
SetConstantValues after HYPRE_IJMatrixAssemble).  The pattern is frozen; the calls of a round are applied in call order
to the stored values, so rounds without constants give, bit for bit, what ONE assembly of all their batches gives
(tests/ij_cases.py: fold).  Host path (HYPRE_MI_IJMatrixAssembleHostOnly); the device path is compared with it in
tests/test_gpu_ij_update.py."""
import numpy as np
import pytest

from tests import ij_cases as cases
from tests import ij_update_cases as upd


def fresh(mi, n, batches):
    return upd.host_snapshot(mi, cases.host_only_matrix(mi, n, [tuple(np.copy(x) if isinstance(x, np.ndarray) else x for x in b) for b in batches]))


def test_three_rounds_equal_one_assembly_of_all_batches(mi_lib):
    mi = mi_lib
    n, pairs, rounds = upd.small_rounds()
    A = cases.new_matrix(mi, 0, n - 1, device=False)
    upd.apply_round(mi, A, rounds[0], host_only=True)
    stamps = [mi.assembly_stamp(A)]
    for k in (1, 2):
        upd.apply_round(mi, A, rounds[k], host_only=True)
        stamps.append(mi.assembly_stamp(A))
        allb = [b for ops in rounds[: k + 1] for b in ops]
        assert cases.same(upd.host_snapshot(mi, A), fresh(mi, n, allb))
        (dia, dja, da), _ = cases.fold(allb, 0, n - 1, 0, n - 1)
        ia, ja, a, _ = mi.parcsr_csr(A, 0)
        assert np.array_equal(ia, dia) and np.array_equal(ja, dja) and np.array_equal(a.view(np.int64), da.view(np.int64))
    assert len(set(stamps)) == 3 and 0 not in stamps  # every closed round is a new assembly
    # the association-sensitive entries of round 2, as the fold of rounds 1 + 2 has them
    (dia, dja, da), _ = cases.fold([b for ops in rounds[:2] for b in ops], 0, n - 1, 0, n - 1)
    row3 = dict(zip(dja[dia[3]:dia[4]].tolist(), da[dia[3]:dia[4]].tolist()))
    assert row3[3] == 0.0 and row3[4] == 0.0 and row3[5] == -6.5


def test_constant_values_land_at_their_place_in_the_order(mi_lib):
    mi = mi_lib
    n, pairs, rounds = upd.small_rounds()
    adds = [b for b in rounds[1] if b[3]]
    A = cases.new_matrix(mi, 0, n - 1, device=False)
    upd.apply_round(mi, A, rounds[0], host_only=True)
    # zero, then Adds: a fresh assembly of those Adds on the same pattern, explicit zeros where nothing was added
    ops = [("const", 0.0)] + adds
    upd.apply_round(mi, A, ops, host_only=True)
    got = upd.host_snapshot(mi, A)
    assert cases.same(got, fresh(mi, n, upd.oracle_batches([ops], pairs)))
    assert np.array_equal(got["ia0"], fresh(mi, n, rounds[0])["ia0"]) and (got["a0"] == 0).any()
    # a constant between two Add batches: what was added before it is gone, what comes after it is added to 2.5
    ops = [adds[0], ("const", 2.5), adds[1]]
    upd.apply_round(mi, A, ops, host_only=True)
    assert cases.same(upd.host_snapshot(mi, A), fresh(mi, n, [upd.const_as_batch(pairs, 2.5), adds[1]]))
    # and a constant as the last call of a round
    upd.apply_round(mi, A, [adds[0], ("const", -1.0)], host_only=True)
    assert cases.same(upd.host_snapshot(mi, A), fresh(mi, n, [upd.const_as_batch(pairs, -1.0)]))


@pytest.mark.parametrize("where", ["diag", "halo_range", "row"])
def test_entries_outside_the_pattern_are_refused_and_change_nothing(mi_lib, where):
    mi = mi_lib
    n, pairs, rounds = upd.small_rounds()
    A = cases.new_matrix(mi, 0, n - 1, device=False)
    upd.apply_round(mi, A, rounds[0], host_only=True)
    before, stamp = upd.host_snapshot(mi, A), mi.assembly_stamp(A)
    missing = next(c for c in range(n) if (3, c) not in pairs)
    r, c = {"diag": (3, missing), "halo_range": (3, n + 5), "row": (n + 2, 1)}[where]
    good = rounds[1][0]
    bad = upd.batch([(pairs[0][0], pairs[0][1], 9.0), (r, c, 1.0), (n + 7, n + 9, 1.0)], True)
    with pytest.raises(mi.HypreError) as e:
        upd.apply_round(mi, A, [good, ("const", 4.0), bad], host_only=True)
    assert f"row {r}," in str(e.value) and f"column {c})" in str(e.value) and "returned 1:" in str(e.value)
    mi.call("HYPRE_ClearAllErrors")
    mi.call("HYPRE_MI_IJMatrixAssembleHostOnly", A.h)  # the refused round is gone: nothing to apply
    assert cases.same(upd.host_snapshot(mi, A), before) and mi.assembly_stamp(A) == stamp
    upd.apply_round(mi, A, rounds[1], host_only=True)
    assert cases.same(upd.host_snapshot(mi, A), fresh(mi, n, rounds[0] + rounds[1])) and mi.assembly_stamp(A) != stamp


def test_assemble_without_a_round_is_a_no_op_and_the_counters_count_rounds(mi_lib):
    mi = mi_lib
    n, pairs, rounds = upd.small_rounds()
    A = cases.new_matrix(mi, 0, n - 1, device=False)
    upd.apply_round(mi, A, rounds[0], host_only=True)
    before, stamp = upd.host_snapshot(mi, A), mi.assembly_stamp(A)
    c0, d0 = mi.counter("ij_value_updates"), mi.counter("ij_device_value_updates")
    mi.call("HYPRE_MI_IJMatrixAssembleHostOnly", A.h)
    assert cases.same(upd.host_snapshot(mi, A), before) and mi.assembly_stamp(A) == stamp
    assert mi.counter("ij_value_updates") == c0
    upd.apply_round(mi, A, rounds[1], host_only=True)
    upd.apply_round(mi, A, rounds[2], host_only=True)
    assert mi.counter("ij_value_updates") == c0 + 2 and mi.counter("ij_device_value_updates") == d0
    # Initialize on an assembled matrix opens a round and keeps the values; closing it gives a new stamp
    now, stamp = upd.host_snapshot(mi, A), mi.assembly_stamp(A)
    A.initialize()
    mi.call("HYPRE_MI_IJMatrixAssembleHostOnly", A.h)
    assert cases.same(upd.host_snapshot(mi, A), now) and mi.assembly_stamp(A) != stamp
    assert mi.counter("ij_value_updates") == c0 + 3
