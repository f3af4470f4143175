"""CPU: the matrix-matrix extended interpolations (interp_type 16 extended, 17 extended+i) built by
the host-only setup, against the numpy restatement of their specification (tests/mm_interp_ref.py), their properties
seen from outside, their two-grid factors beside the library's type 6, the zero denominator, setup reuse and the
replicated multi-rank setup."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from tests import mm_interp_ref as ref
from tests import setup_reuse_cases as rc
from tests.agg2s_common import (ROOT, anisotropic, csr, host_amg, ij_host, random_mmatrix, two_grid_factor,
                                zero_denominator_matrix)
from tests.mm_interp_common import (THETA, marker_before_interpolation, natural_level, one_directional,
                                    same_pattern_close_values, upwind_convection)

WORKER = os.path.join(ROOT, "tests", "mm_interp_dist_worker.py")


def operator(mi, name):
    if name.startswith("lap"):
        stencil, n = (int(x) for x in name[3:].split("_"))
        return mi.build_laplace_system_host(n, n, n, stencil, 0, 1)[0]
    M = {"aniso": anisotropic, "randmm": random_mmatrix, "upwind": upwind_convection, "onedir": one_directional}[name]()
    return ij_host(mi, M)


def test_symbol_declared_and_exported(mi_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "HYPRE_mi_ext.h")).read(), flags=re.S)
    assert re.search(r"HYPRE_Int\s+HYPRE_MI_MMInterpOp\s*\(", text)
    assert hasattr(mi_lib.lib(), "HYPRE_MI_MMInterpOp") and hasattr(mi_lib, "mm_interp_op")


def test_types_16_and_17_are_accepted_and_15_is_still_refused(mi_lib):
    mi = mi_lib
    A, _ = mi.build_laplace_system_host(6, 6, 6, 7, 0, 1)
    for t in (16, 17):
        amg = host_amg(mi, A, interp_type=t)
        assert amg.num_levels >= 2
        # "another interpolation type": the census of sk::interp is all zeros, the flag is set
        assert amg.interp_census(0)["host"] and not amg.interp_census(0)["fell_back"]
    amg = mi.BoomerAMG(print_level=0, interp_type=15)
    with pytest.raises(mi.HypreError, match=r"interp_type 15 is not implemented \(.*16 extended and 17 extended\+i"):
        mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
    mi.call("HYPRE_ClearAllErrors")


VARIANTS = [dict(true_pmax_elmts=0), dict(true_pmax_elmts=4), dict(true_pmax_elmts=0, trunc_factor=0.2),
            dict(true_pmax_elmts=4, trunc_factor=0.2), dict(true_pmax_elmts=4, agg_num_levels=1)]


@pytest.mark.parametrize("kw", VARIANTS, ids=lambda kw: "-".join("%s%s" % (k.replace("true_", ""), v) for k, v in kw.items()))
@pytest.mark.parametrize("name", ["lap7_12", "lap27_10", "aniso", "randmm", "upwind"])
@pytest.mark.parametrize("t", [16, 17])
def test_p_equals_the_restatement_on_every_level_that_is_not_aggressive(mi_lib, t, name, kw):
    mi = mi_lib
    amg = host_amg(mi, operator(mi, name), interp_type=t, **kw)
    first = kw.get("agg_num_levels", 0)
    assert amg.num_levels - 1 > first, "no level for the new type"
    for l in range(first, amg.num_levels - 1):
        A, cf, P = natural_level(amg, l)
        assert set(np.unique(cf)) <= {1, -1}  # the marker handed on has -3 -> -1
        strong = ref.strength_rows(A, THETA)
        m = marker_before_interpolation(cf, strong)
        Pref = ref.mm_interp(A, strong, m, t, trunc_factor=kw.get("trunc_factor", 0.0), pmax=kw["true_pmax_elmts"])
        same_pattern_close_values(P, Pref)
        if kw["true_pmax_elmts"]:
            assert np.diff(P.indptr).max() <= kw["true_pmax_elmts"]
        assert amg.interp_census(l)["host"]


@pytest.mark.parametrize("t,name,kw", [(16, "lap7_12", dict(true_pmax_elmts=4)), (17, "lap7_12", dict(true_pmax_elmts=4)),
                                       (17, "aniso", dict(true_pmax_elmts=0)), (16, "aniso", dict(true_pmax_elmts=4, trunc_factor=0.2)),
                                       (17, "randmm", dict(true_pmax_elmts=4)), (17, "upwind", dict(true_pmax_elmts=0))])
def test_properties_seen_from_outside(mi_lib, t, name, kw):
    mi = mi_lib
    amg = host_amg(mi, operator(mi, name), interp_type=t, **kw)
    seen_zero_sum_rows = 0
    for l in range(amg.num_levels - 1):
        A, P, cf = csr(amg, l, 0), csr(amg, l, 2), amg.level_cf(l)
        n, nc = P.shape
        assert nc == int((cf == 1).sum())
        # C rows are unit rows (C-first ordering: C point q is coarse unknown q of the level's natural numbering, which
        # the next level's own C-first ordering then permutes)
        permc = amg.level_perm(l + 1)
        rows_c = np.flatnonzero(cf == 1)
        assert np.array_equal(np.diff(P.indptr)[rows_c], np.ones(len(rows_c), dtype=int))
        assert np.array_equal(P.data[P.indptr[rows_c]], np.ones(len(rows_c)))
        assert np.array_equal(permc[P.indices[P.indptr[rows_c]]], np.arange(nc))
        # a row sums to 1 where row i and the rows of its neighbours sum to zero (truncation keeps the row sum)
        rs = np.abs(np.asarray(A.sum(axis=1)).ravel()) > 1e-12 * np.abs(A.diagonal())
        G = (abs(A) + sp.identity(n)).tocsr()
        G.data[:] = 1.0
        ok = ((G @ rs.astype(float)) == 0) & (np.diff(P.indptr) > 0)
        seen_zero_sum_rows += int(ok.sum())
        sums = np.asarray(P.sum(axis=1)).ravel()
        assert np.all(np.abs(sums[ok] - 1.0) < 1e-12), np.abs(sums[ok] - 1.0).max()
        # Galerkin: A_c = P^T A P, in the next level's ordering
        Ac = csr(amg, l + 1, 0)
        assert abs(Ac - (P.T @ A @ P).tocsr()).max() <= 1e-12 * abs(Ac).max()
        assert abs(csr(amg, l, 3) - P.T).nnz == 0
    if name in ("lap7_12", "aniso"):
        assert seen_zero_sum_rows > 0


@pytest.mark.parametrize("t", [16, 17])
@pytest.mark.parametrize("name", ["lap27_10", "upwind", "randmm"])
def test_the_hierarchy_of_minus_a_has_the_bits_of_p(mi_lib, oc, t, name):
    mi = mi_lib
    Mp = {"lap27_10": lambda: rc.system(oc, "lap27_10"), "upwind": upwind_convection, "randmm": random_mmatrix}[name]()
    kw = dict(interp_type=t, true_pmax_elmts=4)
    a_plus, a_minus = host_amg(mi, ij_host(mi, Mp), **kw), host_amg(mi, ij_host(mi, -Mp), **kw)
    assert a_plus.num_levels == a_minus.num_levels >= 3
    for l in range(a_plus.num_levels - 1):
        assert rc.same_csr(a_plus.level_csr(l, 2), a_minus.level_csr(l, 2)), l
        assert np.array_equal(a_plus.level_cf(l), a_minus.level_cf(l))


def test_type_17_equals_type_16_where_the_strong_f_f_couplings_are_one_directional(mi_lib):
    mi = mi_lib
    M = one_directional()
    a16 = host_amg(mi, ij_host(mi, M), interp_type=16, max_levels=2)
    a17 = host_amg(mi, ij_host(mi, M), interp_type=17, max_levels=2)
    A, cf, P16 = natural_level(a16, 0)
    _, cf17, P17 = natural_level(a17, 0)
    assert np.array_equal(cf, cf17)
    # the case is there: F rows with a strong F neighbour that has strong C neighbours of its own
    strong = ref.strength_rows(A, THETA)
    pairs = sum(1 for i in range(A.shape[0]) if cf[i] == -1 for k in strong[i]
                if cf[k] == -1 and any(cf[l] == 1 for l in strong[k]))
    assert pairs > 20, pairs
    assert all(A[k, i] == 0.0 for i in range(A.shape[0]) for k in strong[i])
    same_pattern_close_values(P17, P16)
    # and where they are not (the 7-point operator) the two types differ
    b16 = host_amg(mi, operator(mi, "lap7_6"), interp_type=16, max_levels=2)
    b17 = host_amg(mi, operator(mi, "lap7_6"), interp_type=17, max_levels=2)
    assert abs(csr(b16, 0, 2) - csr(b17, 0, 2)).max() > 1e-3


def test_two_grid_factors_beside_type_6(mi_lib):
    """Level 0 as a two-level setup (max_levels 2, P_max_elmts 4), one symmetric Gauss-Seidel sweep.  The restatement
    alone gives tg17 / tg6 = 0.997, 1.003, 1.000, 1.008 and tg17 / tg16 = 0.81 (7-point) and 0.57 (anisotropic)."""
    mi = mi_lib
    tg = {}
    for name in ("lap7_10", "lap27_8", "aniso", "randmm"):
        for t in (6, 16, 17):
            amg = host_amg(mi, operator(mi, name), interp_type=t, true_pmax_elmts=4, max_levels=2)
            tg[name, t] = two_grid_factor(csr(amg, 0, 0), csr(amg, 0, 2))
        print("two-grid factor %-8s: type 6 %.4f, type 16 %.4f, type 17 %.4f" % (name, tg[name, 6], tg[name, 16], tg[name, 17]))
    for name in ("lap7_10", "lap27_8", "aniso", "randmm"):
        assert tg[name, 17] <= 1.05 * tg[name, 6], (name, tg[name, 17], tg[name, 6])
    assert tg["lap7_10", 17] <= 0.9 * tg["lap7_10", 16]
    assert tg["aniso", 17] <= 0.75 * tg["aniso", 16]


@pytest.mark.parametrize("t", [16, 17])
def test_zero_denominator_fails_setup_naming_type_level_and_row(mi_lib, t):
    """d_i = 0 with a non-empty numerator (tests/agg2s_common.py zero_denominator_matrix)."""
    mi = mi_lib
    A = ij_host(mi, zero_denominator_matrix())
    amg = mi.BoomerAMG(print_level=0, interp_type=t)
    with pytest.raises(mi.HypreError, match=r"interp_type %d\) on level 0: row \d+ has a zero denominator" % t):
        mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
    mi.call("HYPRE_ClearAllErrors")
    # type 6 on the same matrix does not care
    host_amg(mi, A)


def test_setup_reuse_refreshes_and_keeps_p(mi_lib, oc):
    from tests import ij_cases as cases
    from tests import ij_update_cases as upd

    mi = mi_lib
    M0 = rc.system(oc, "lap7_8")
    M1 = rc.changed(M0, "d")
    A = cases.host_only_matrix(mi, M0.shape[0], [rc.triples(M0) + (False,)])
    amg = mi.BoomerAMG(print_level=0, interp_type=17, true_pmax_elmts=4, setup_reuse=1)
    mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
    assert amg.setup_kind() == (1, 1) and amg.num_levels >= 3
    before = rc.snapshot(amg)
    upd.apply_round(mi, A, [rc.triples(M1) + (False,)], host_only=True)
    mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
    assert amg.setup_kind() == (2, 0)
    after = rc.snapshot(amg)
    assert len(before) == len(after)
    for b, a in zip(before[:-1], after[:-1]):
        assert rc.same_csr(b["P"], a["P"]) and rc.same_csr(b["R"], a["R"]) and np.array_equal(b["cf"], a["cf"])
    assert not rc.same_csr(before[1]["A"], after[1]["A"]) and rc.same_csr(before[1]["A"], after[1]["A"], values=False)


def test_replicated_setup_on_gloo_ranks_gives_the_single_rank_hierarchy():
    env = dict(os.environ, MI_HYPRE_HOST_THREADS="2", OMP_NUM_THREADS="1", MI_HYPRE_LOCALITY_ORDER="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", "30957", WORKER, "--grid", "12", "--interp", "17"]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    assert p.stdout.count("mm_interp rank ok") == 2, p.stdout[-4000:]
