"""CPU: FSAI with the adaptive pattern (fsai_algo_type 4; DESIGN.md section 3, "FSAI (adaptive pattern)").  The numpy
restatement of the specification (tests/fsai_adaptive_ref.py) is checked against the identities it must satisfy, and
the library's host routine -- HYPRE_MI_FSAIAdaptiveOp with on_host = 1, no device -- against the restatement on every
case of tests/fsai_adaptive_cases.py: patterns exactly, values within 1e-12 of max |G|, the info[] counts, every
refusal, and the condition number the adaptive pattern buys on an anisotropic operator."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from tests import fsai_adaptive_cases as fc
from tests import fsai_adaptive_ref as ref
from tests import fsai_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = [("lap7_8", 3, 5, 1e-3), ("lap7_8", 5, 3, 0.0), ("lap7_8", 2, 3, 0.2), ("aniso_8", 3, 1, 0.0),
          ("ragged_small", 9, 7, 0.0), ("ragged_small", 31, 1, 1e-3), ("short_rows", 4, 8, 0.0)]


def test_symbols_are_declared_and_exported(mi_lib):
    def text(name):
        return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    for sym in ("HYPRE_MI_FSAIAdaptiveOp", "HYPRE_MI_BoomerAMGGetLevelFSAIInfo", "HYPRE_MI_FSAIGetSetupInfo"):
        assert re.search(r"HYPRE_Int\s+%s\s*\(" % sym, text("HYPRE_mi_ext.h")), sym
        assert hasattr(mi_lib.lib(), sym), sym
    assert hasattr(mi_lib, "fsai_adaptive_op") and hasattr(mi_lib.BoomerAMG, "level_fsai_info")
    assert hasattr(mi_lib.FSAI, "setup_info")


@pytest.mark.parametrize("name", ["lap7_8", "lap27_8", "aniso_8", "ragged_small", "short_rows", "diagonal"])
def test_identities_of_the_restatement(name):
    B = fc.matrix(name)
    G, info = fc.reference(name, *fc.DEFAULTS)
    s, t, _ = fc.DEFAULTS
    assert sp.tril(G).nnz == G.nnz and info["max_row"] <= s * t + 1
    W = (G @ B).toarray()
    scale = np.abs(G.toarray()).max() * np.abs(B.toarray()).max()
    # diag(G B G^T) = 1, and (G B)_ij = 0 on the pattern below the diagonal
    assert np.abs((G @ B @ G.T).diagonal() - 1.0).max() < 1e-12
    for i in range(B.shape[0]):
        P = G.indices[G.indptr[i]:G.indptr[i + 1]]
        assert P[-1] == i and np.all(np.diff(P) > 0)
        assert np.abs(W[i, P[:-1]]).max(initial=0.0) < 1e-12 * scale
    # G is static FSAI on the pattern the growth found
    Gs = fsai_ref.factor(B, pat=info["pattern"])
    assert np.array_equal(Gs.indices, G.indices) and np.array_equal(Gs.data, G.data)
    # psi never increases by more than rounding
    for ps in info["psi"]:
        assert all(b <= a * (1.0 + 1e-14) for a, b in zip(ps, ps[1:]))


def test_a_bound_that_holds_the_whole_row_gives_the_inverse():
    """s * t >= i for every row: the pattern is the whole lower triangle wherever the gradient does not vanish, and for
    a matrix whose inverse factor is full G^T G = B^-1."""
    rng = np.random.default_rng(7)
    n = 20
    X = rng.standard_normal((n, n))
    B = sp.csr_matrix(X @ X.T + n * np.eye(n))
    G, info = ref.factor(B, n, 1, 0.0)
    assert info["max_row"] == n and list(np.diff(G.indptr)) == list(range(1, n + 1))
    assert np.abs((G.T @ G).toarray() - np.linalg.inv(B.toarray())).max() < 1e-12


def test_the_cases_hold_what_they_are_for():
    _, info = fc.reference("lap7_8", *fc.DEFAULTS)
    assert all(info["stops"][k] > 0 for k in info["stops"])  # all three stop reasons on one operator
    _, info = fc.reference("diagonal", *fc.DEFAULTS)
    assert info["stops"][ref.STOP_NO_CANDIDATE] == 37 and info["max_row"] == 1 and info["max_candidates"] == 0
    _, info = fc.reference("short_rows", 4, 8, 0.0)
    assert 0 < info["max_candidates"] < 8  # fewer candidates than max_step_size
    _, info = fc.reference("ragged_small", 9, 7, 0.0)
    assert info["max_row"] == 64 and info["max_candidates"] > 64
    assert fc.matrix("five_rows").shape[0] % 4 != 0
    for name, (_, row, _) in fc.FAILING.items():
        with pytest.raises(ref.RowFailure) as e:
            ref.factor(fc.matrix(name))
        assert e.value.row == row


@pytest.mark.parametrize("name", list(fc.CASES))
def test_host_routine_equals_the_restatement(mi_lib, name):
    Gr, rinfo = fc.reference(name, *fc.DEFAULTS)
    G, info = mi_lib.fsai_adaptive_op(fc.matrix(name), *fc.DEFAULTS, host=True)
    fc.same_G(fc.as_csr(G), Gr)
    fc.same_counts(info, rinfo)
    assert info["overflow_rows"] == 0


@pytest.mark.parametrize("name,s,t,tau", PARAMS)
def test_host_routine_equals_the_restatement_for_other_parameters(mi_lib, name, s, t, tau):
    Gr, rinfo = fc.reference(name, s, t, tau)
    G, info = mi_lib.fsai_adaptive_op(fc.matrix(name), s, t, tau, host=True)
    fc.same_G(fc.as_csr(G), Gr)
    fc.same_counts(info, rinfo)
    assert info["max_row"] <= s * t + 1


def test_host_routine_does_not_depend_on_the_thread_count_or_table_slots(mi_lib, monkeypatch):
    B = fc.matrix("ragged_small")
    G0, i0 = mi_lib.fsai_adaptive_op(B, 5, 3, 1e-3, host=True)
    monkeypatch.setenv("MI_HYPRE_HOST_THREADS", "3")
    G1, i1 = mi_lib.fsai_adaptive_op(B, 5, 3, 1e-3, table_slots=8, host=True)
    assert i0 == i1 and all(np.array_equal(u, v) for u, v in zip(G0[:3], G1[:3]))


def test_the_op_names_every_refusal(mi_lib):
    B = fc.matrix("five_rows")
    for kw, msg in ((dict(max_steps=0), "must be"), (dict(max_step_size=0), "must be"),
                    (dict(max_steps=9, max_step_size=8), "not implemented"), (dict(max_steps=64, max_step_size=1), "must be <= 64"),
                    (dict(kap_tolerance=-1e-3), "must be"), (dict(kap_tolerance=float("nan")), "must be"),
                    (dict(kap_tolerance=float("inf")), "must be"), (dict(table_slots=3), "power of two")):
        with pytest.raises(mi_lib.HypreError, match=msg):
            mi_lib.fsai_adaptive_op(B, host=True, **kw)
        mi_lib.call("HYPRE_ClearAllErrors")
    mi_lib.fsai_adaptive_op(B, 63, 1, 0.0, host=True)  # the largest bound
    for name, (_, row, what) in fc.FAILING.items():
        with pytest.raises(mi_lib.HypreError, match=r"row %d \(%s" % (row, what)) as e:
            mi_lib.fsai_adaptive_op(fc.matrix(name), host=True)
        assert e.value.info["status"] == 2 and e.value.info["bad_row"] == row
        mi_lib.call("HYPRE_ClearAllErrors")


def test_the_adaptive_pattern_conditions_an_anisotropic_operator_better():
    """cond(G B G^T) on the (1, 1, 100) operator: 3 steps of 1 entry (4 entries per row) against the static pattern of
    the same size (theta 0.01, k = 1); both from numpy."""
    B = fc.matrix("aniso_8")

    def cond(G):
        W = (G @ B @ G.T).toarray()
        ev = np.linalg.eigvalsh(0.5 * (W + W.T))
        return ev[-1] / ev[0]
    Ga = fc.reference("aniso_8", 3, 1, 0.0)[0]
    Gs = fsai_ref.factor(B, 0.01, 1)
    print("entries per row %.2f / %.2f, cond %.2f / %.2f" % (Ga.nnz / 512, Gs.nnz / 512, cond(Ga), cond(Gs)))
    assert cond(Ga) < cond(Gs)
