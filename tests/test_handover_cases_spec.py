"""CPU: what the operators of tests/handover_cases.py are for, from the oracle's hierarchy at the app defaults (PMIS,
strong threshold 0.57): the C-first ordering, the number of C rows and its remainder mod 8 (a tile can end exactly at nc
only when it is 0), the C rows with an off-diagonal C column (the rows the hand-over's Setup flags), and whether level
0 can be stored with a value dictionary (at most 256 distinct values) or stays fp64.  The GPU tests of the hand-over
(tests/test_gpu_c_row_handover_paths.py) rely on these properties; if a generator drifts, this fails first."""
import numpy as np
import pytest

from tests import handover_cases as hc

# nc % 8 of every case, written out: the edge cases are chosen by it
NC_MOD_8 = {"lap7_9": 7, "lap7_12": 4, "lap7_12_scaled_sym": 4, "lap7_12_scaled_nonsym": 4, "lap7_19": 0,
            "lap7_19_scaled_sym": 0, "lap7_30": 4, "lap27_12": 3, "aniso16_8": 7, "aniso16_8_scaled_nonsym": 6,
            "aniso16_4": 0, "lap7_22": 1, "aniso22_11": 3}
# the cases level 0 of which is stored with a value dictionary: few distinct values AND at least DICTIONARY_MIN_NNZ
# stored entries (the library leaves smaller operators in fp64)
DICTIONARY = {"lap7_30", "lap7_22", "aniso22_11"}


def test_every_case_is_listed():
    assert set(NC_MOD_8) == set(hc.CASES)


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_recorded_properties(oc, name):
    _, n, nc_want, flagged_want, many_values = hc.CASES[name]
    M = hc.case(name)
    assert M.shape == (n, n) and M.has_sorted_indices
    amg = oc.Amg(oc.Csr.from_scipy(M), oc.default_params())
    A0, cf = amg.level_A(0).to_scipy(), amg.level_cf(0)
    nc, flagged = hc.flagged_rows(A0, cf)
    distinct = len(np.unique(M.data))
    print(f"{name}: n {n}, nc {nc} (nc % 8 = {nc % 8}), flagged {int(flagged.sum())}, distinct values {distinct}")
    assert np.all(cf[:nc] == 1) and not np.any(cf[nc:] == 1)
    assert nc == nc_want
    assert nc % 8 == NC_MOD_8[name]
    assert int(flagged.sum()) == flagged_want
    assert (distinct > 256) == many_values
    assert (distinct <= 256 and M.nnz >= hc.DICTIONARY_MIN_NNZ) == (name in DICTIONARY)
    # level 0 is the operator itself in the C-first ordering
    p = amg.level_perm(0).astype(np.int64)
    assert abs(A0 - M[p][:, p]).max() == 0.0


def test_aniso_is_the_half_anisotropic_operator():
    assert abs(hc.aniso(16, 8) - hc.half_anisotropic()).max() == 0.0
    assert abs(hc.aniso(16, 8, 0.25) - hc.half_anisotropic(16, 0.25)).max() == 0.0


def test_scaled_draws():
    M = hc.lap7(4)
    n = M.shape[0]
    rng = np.random.default_rng(3)
    d1 = 1.0 + 0.2 * (2.0 * rng.random(n) - 1.0)
    d2 = 1.0 + 0.2 * (2.0 * rng.random(n) - 1.0)
    S, N = hc.scaled(M), hc.scaled(M, sym=False)
    assert np.array_equal(S.indices, M.indices) and np.array_equal(N.indptr, M.indptr)
    D = M.toarray()
    assert np.allclose(S.toarray(), d1[:, None] * D * d1[None, :], rtol=1e-15, atol=0.0)
    assert np.allclose(N.toarray(), d1[:, None] * D * d2[None, :], rtol=1e-15, atol=0.0)
    # (d1_i m) d1_j and (d1_j m) d1_i round differently: symmetric to two roundings of the largest entry
    assert abs(S - S.T).max() <= 2 * 2.0 ** -52 * abs(S).max() and abs(N - N.T).max() > 1e-3
    assert abs(hc.scaled(M, seed=4) - S).max() > 0.0


def test_explicit_zeros_are_stored():
    M = hc.lap7(4)
    pairs = [(0, 5), (2, 63)]
    Z = hc.with_explicit_zeros(M, pairs)
    assert Z.nnz == M.nnz + 4 and abs(Z - M).max() == 0.0
    for i, j in pairs:
        for r, c in ((i, j), (j, i)):
            cols = Z.indices[Z.indptr[r]:Z.indptr[r + 1]]
            assert c in cols and Z[r, c] == 0.0
