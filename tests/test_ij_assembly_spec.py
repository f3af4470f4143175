"""CPU: the specification of HYPRE_IJMatrixAssemble.  The host assembly (HYPRE_MI_IJMatrixAssembleHostOnly), read
through HYPRE_MI_ParCSRGetCSR, against a plain-Python statement of the fold (tests/ij_cases.py: a dict keyed by (row,
column), walked in submission order) -- the device assembly is then compared with the host assembly bit for bit
(tests/test_gpu_ij_device_assembly.py)."""
import numpy as np

from tests import ij_cases as cases


def test_case_has_what_it_is_meant_to_have():
    n, batches = cases.duplicates_small()
    assert n == 40 and [b[3] for b in batches] == [False, True, False]
    pairs = {}
    for rows, cols, vals, _ in batches:
        for r, c in zip(rows.tolist(), cols.tolist()):
            pairs[(r, c)] = pairs.get((r, c), 0) + 1
    assert set(pairs.values()) == {1, 2, 3, 4}
    assert 17 not in {r for r, _ in pairs}  # an empty row
    # the sums depend on the association: (0 + 1e16 + 1) - 1e16 is 0 in submission order, 1 in another
    (dia, dja, da), _ = cases.fold(batches, 0, n - 1, 0, n - 1)
    row3 = dict(zip(dja[dia[3]:dia[4]].tolist(), da[dia[3]:dia[4]].tolist()))
    assert row3[3] == 0.0 and row3[4] == 1.0 and row3[5] == -4.0
    assert (0.0 + cases.BIG - cases.BIG) + 1.0 == 1.0
    row9 = dict(zip(dja[dia[9]:dia[10]].tolist(), da[dia[9]:dia[10]].tolist()))
    assert row9[9] == 0.0  # an explicit zero stays


def test_host_assembly_equals_the_python_fold(mi_lib):
    mi = mi_lib
    n, batches = cases.duplicates_small()
    A = cases.host_only_matrix(mi, n, batches)
    (dia, dja, da), (oia, oj, oa) = cases.fold(batches, 0, n - 1, 0, n - 1)
    ia, ja, a, shape = mi.parcsr_csr(A, 0)
    assert shape == (n, n)
    assert np.array_equal(ia, dia) and np.array_equal(ja, dja)
    assert np.array_equal(a.view(np.int64), da.view(np.int64))
    assert ia[18] == ia[17]
    ia1, ja1, a1, shape1 = mi.parcsr_csr(A, 1)
    assert shape1 == (n, 0) and np.array_equal(ia1, oia) and len(ja1) == 0 and len(mi.parcsr_colmap(A)) == 0


def test_host_assembly_splits_diag_and_offd_like_the_fold(mi_lib):
    """the same entries on a matrix whose column range is [10, 29]: the rest forms the offd block, whose compressed
    columns map to sorted global ids"""
    mi = mi_lib
    n, batches = cases.duplicates_small()
    A = cases.new_matrix(mi, 0, n - 1, 10, 29, device=False)
    cases.stage(mi, A, batches, device=False)
    # This test leans on something incidental: one rank cannot own a halo block, so the call below is refused -- but
    # only by the halo plan, AFTER the assembly has filled diag, offd and the column map, and a refused call leaves
    # them in place.  A split that assembles cleanly needs a second rank; the ranks of
    # tests/ij_device_dist_worker.py compare such blocks (device against host assembly) on the GPU.  Should the halo
    # plan come to accept this matrix, drop the rc check; should a refused assembly come to clear the matrix, this
    # case has to move to a two-rank CPU worker.
    rc = mi.lib().HYPRE_MI_IJMatrixAssembleHostOnly(A.h)
    assert rc != 0 and b"outside the single rank's range" in mi.lib().HYPRE_MI_LastErrorMessage()
    mi.call("HYPRE_ClearAllErrors")
    (dia, dja, da), (oia, oj, oa) = cases.fold(batches, 0, n - 1, 10, 29)
    ia, ja, a, shape = mi.parcsr_csr(A, 0)
    assert shape == (n, 20) and np.array_equal(ia, dia) and np.array_equal(ja, dja)
    assert np.array_equal(a.view(np.int64), da.view(np.int64))
    ia1, ja1, a1, _ = mi.parcsr_csr(A, 1)
    cm = mi.parcsr_colmap(A)
    assert np.array_equal(cm, np.unique(oj)) and np.array_equal(ia1, oia)
    assert np.array_equal(cm[ja1], oj) and np.array_equal(a1.view(np.int64), oa.view(np.int64))
