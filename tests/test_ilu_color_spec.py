"""CPU: the multicolour ordering of the ILU (local_reordering 2).  The interface is declared and
exported, and the Python reference (tests/ilu_color_ref.py) has, on every operator of tests/ilu_color_cases.py, the
properties the specification promises: a proper colouring of D + D^T with at most max degree + 1 colours, perm a
permutation sorted by (colour, index), and at fill 0 no more level sets per factor than colours."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from tests import ilu_color_cases as cc
from tests import ilu_color_ref as ref
from tests import ilu_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_and_exported(mi_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "HYPRE_mi_ext.h")).read(), flags=re.S)
    for sym in ("HYPRE_MI_ILUGetOrdering", "HYPRE_MI_BoomerAMGGetLevelILUOrdering"):
        assert re.search(r"HYPRE_Int\s+%s\s*\(" % sym, text), sym
        assert hasattr(mi_lib.lib(), sym), sym
    assert hasattr(mi_lib.ILU, "ordering") and hasattr(mi_lib.BoomerAMG, "level_ilu_ordering")


def test_fmix32_is_the_murmur3_finaliser():
    # fmix32(0) = 0, it is a bijection on 32 bits (no two of 2^16 inputs agree), and one value spelt out in plain ints
    assert int(ref.fmix32(0)) == 0
    w = ref.fmix32(np.arange(1 << 16))
    assert len(np.unique(w)) == 1 << 16
    h = 12345
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    assert int(ref.fmix32(12345)) == h and int(ref.weights(12345)[12344]) == h


@pytest.mark.parametrize("name", cc.NAMES)
def test_the_reference_is_a_proper_colouring_in_few_colours(name):
    o = cc.ordering(name)
    G = o.G.tocoo()
    assert np.all(o.colour >= 0)
    assert np.all(o.colour[G.row] != o.colour[G.col])
    assert o.ncolours <= o.max_degree + 1
    # first fit: every row holds the smallest colour its earlier neighbours leave, so every smaller one is a neighbour's
    for i in range(o.n):
        nb = o.G.indices[o.G.indptr[i]:o.G.indptr[i + 1]]
        assert set(range(o.colour[i])) <= set(o.colour[nb].tolist())
    assert 1 <= o.rounds <= o.n


@pytest.mark.parametrize("name", cc.NAMES)
def test_perm_is_a_permutation_sorted_by_colour_then_index(name):
    o = cc.ordering(name)
    assert np.array_equal(np.sort(o.perm), np.arange(o.n))
    key = o.colour[o.perm].astype(np.int64) * o.n + o.perm
    assert np.all(np.diff(key) > 0)


@pytest.mark.parametrize("name", cc.NAMES)
def test_level_sets_of_the_permuted_pattern_are_at_most_the_colours(name):
    o = cc.ordering(name)
    B = o.permuted(cc.matrix(name))
    lower, upper = ilu_ref.level_sets(B.indptr.astype(np.int64), B.indices)
    assert lower <= o.ncolours and upper <= o.ncolours


def test_the_counts_of_the_named_cases():
    assert cc.ordering("diagonal").ncolours == 1 and cc.ordering("diagonal").rounds == 1
    assert cc.ordering("one").ncolours == 1 and cc.ordering("one").rounds == 1
    assert cc.ordering("dense70").ncolours == 70  # the dense block is a clique of 70, the rows beside it have degree <= 3
    assert cc.ordering("path").ncolours <= 3
    M = cc.matrix("upwind")
    assert (M != M.T).nnz > 0 and (abs(M) > 0).multiply(abs(M.T) > 0).nnz == M.shape[0]  # no a_ij has its a_ji
    assert np.diff(cc.matrix("ragged").indptr).max() > 256
    off = cc.matrix("convdiff") - sp.diags(cc.matrix("convdiff").diagonal())
    assert off.data.min() < 0 < off.data.max()
    # natural order of the 7-point 16^3 operator: 3 n - 2 level sets per factor
    L = cc.matrix("lap7_16")
    assert ilu_ref.level_sets(L.indptr.astype(np.int64), L.indices) == (46, 46)
