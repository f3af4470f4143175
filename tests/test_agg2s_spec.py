"""CPU: the two-stage extended interpolation of aggressive levels (agg_interp_type 5) built by the
host-only setup, against the numpy restatement of its specification (tests/agg2s_ref.py), its properties seen from
outside, its two-grid factor beside multipass's, and the replicated multi-rank setup."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from tests import agg2s_ref
from tests.agg2s_common import (ROOT, anisotropic, csr, host_amg, ij_host, random_mmatrix, two_grid_factor,
                                zero_denominator_matrix)

WORKER = os.path.join(ROOT, "tests", "agg2s_dist_worker.py")
THETA = 0.57  # strong_threshold of mi.BoomerAMG's defaults (the app's)


def operator(mi, name):
    if name == "lap7_12":
        return mi.build_laplace_system_host(12, 12, 12, 7, 0, 1)[0]
    if name == "lap27_10":
        return mi.build_laplace_system_host(10, 10, 10, 27, 0, 1)[0]
    if name == "aniso":
        return ij_host(mi, anisotropic())
    return ij_host(mi, random_mmatrix())


def natural_level(amg, l):
    """A of level l, the two stage markers and P in the level's NATURAL numbering (the one the hierarchy is built in:
    the specification's "stored order"; level_csr reports C-first renumbered copies)."""
    perm = amg.level_perm(l).astype(np.int64)       # perm[new] = old
    permc = amg.level_perm(l + 1).astype(np.int64)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    A = csr(amg, l, 0)[inv][:, inv].tocsr()
    A.sort_indices()
    m1r, m2r = amg.level_agg_markers(l)
    m1, m2 = np.empty_like(m1r), np.empty_like(m2r)
    m1[perm], m2[perm] = m1r, m2r
    # (explicit zeros, if any, must survive the renumbering: work on the arrays)
    return A, m1, m2, _permute_keep_zeros(csr(amg, l, 2), inv, permc)


def _permute_keep_zeros(P, row_new_of_old, col_old_of_new):
    """rows: natural row i = reported row row_new_of_old[i]; columns: reported column q = natural column col_old_of_new[q]"""
    indptr, indices, data = [0], [], []
    for i in range(P.shape[0]):
        r = row_new_of_old[i]
        c = col_old_of_new[P.indices[P.indptr[r]:P.indptr[r + 1]]]
        v = P.data[P.indptr[r]:P.indptr[r + 1]]
        o = np.argsort(c, kind="stable")
        indices += list(c[o])
        data += list(v[o])
        indptr.append(len(indices))
    return sp.csr_matrix((np.array(data, dtype=float), np.array(indices, dtype=np.int64), np.array(indptr)), shape=P.shape)


def same_pattern_close_values(P, Q, rtol=1e-13):
    assert P.shape == Q.shape, (P.shape, Q.shape)
    assert np.array_equal(P.indptr, Q.indptr) and np.array_equal(P.indices, Q.indices), "patterns differ"
    err = np.abs(P.data - Q.data)
    print("max relative difference %.3e over %d entries" % ((err / np.maximum(np.abs(Q.data), 1e-300)).max(initial=0.0), len(err)))
    assert np.all(err <= rtol * np.abs(Q.data))


def test_symbols_declared_and_exported(mi_lib):
    text = ""
    for h in ("HYPRE_parcsr_ls.h", "HYPRE_mi_ext.h"):
        text += re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
    for name in ("HYPRE_BoomerAMGSetAggP12MaxElmts", "HYPRE_BoomerAMGSetAggP12TruncFactor",
                 "HYPRE_MI_BoomerAMGGetLevelAggMarkers", "HYPRE_MI_BoomerAMGSetKeepAggMarkers"):
        assert re.search(r"HYPRE_Int\s+" + name + r"\s*\(", text), name
        assert hasattr(mi_lib.lib(), name), name


def test_type_5_is_accepted_and_the_other_values_still_refused(mi_lib):
    mi = mi_lib
    A, rhs = mi.build_laplace_system_host(6, 6, 6, 7, 0, 1)
    amg = host_amg(mi, A, agg_num_levels=1, agg_interp_type=5)
    assert amg.num_levels >= 2
    for t in (2, 3, 6, 7):
        amg = mi.BoomerAMG(print_level=0, agg_num_levels=1, agg_interp_type=t)
        with pytest.raises(mi.HypreError, match="agg_interp_type %d is not implemented" % t):
            mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
        mi.call("HYPRE_ClearAllErrors")
    # the stage markers are kept on request only
    unkept = mi.BoomerAMG(print_level=0, agg_num_levels=1, agg_interp_type=5)
    mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", unkept.h, A.par)
    with pytest.raises(mi.HypreError, match="SetKeepAggMarkers"):
        unkept.level_agg_markers(0)
    mi.call("HYPRE_ClearAllErrors")
    # the markers of a level the two-stage interpolation did not build are not there to ask for
    plain = host_amg(mi, A, agg_num_levels=1)
    with pytest.raises(mi.HypreError, match="two-stage"):
        plain.level_agg_markers(0)
    mi.call("HYPRE_ClearAllErrors")


VARIANTS = [dict(agg_num_levels=1), dict(agg_num_levels=2), dict(agg_num_levels=1, agg_pmax_elmts=4),
            dict(agg_num_levels=1, agg_pmax_elmts=4, agg_p12_max_elmts=4),
            dict(agg_num_levels=2, agg_pmax_elmts=4, agg_p12_max_elmts=4),
            dict(agg_num_levels=1, agg_trunc_factor=0.2, agg_p12_trunc_factor=0.1)]


@pytest.mark.parametrize("kw", VARIANTS, ids=lambda kw: "-".join("%s%s" % (k.replace("agg_", ""), v) for k, v in kw.items()))
@pytest.mark.parametrize("name", ["lap7_12", "lap27_10", "aniso", "randmm"])
def test_p_equals_the_restatement_on_every_aggressive_level(mi_lib, name, kw):
    mi = mi_lib
    amg = host_amg(mi, operator(mi, name), agg_interp_type=5, **kw)
    nagg = min(kw["agg_num_levels"], amg.num_levels - 1)
    assert nagg >= 1
    for l in range(nagg):
        A, m1, m2, P = natural_level(amg, l)
        assert set(np.unique(m1)) <= {1, -1, -3} and set(np.unique(m2)) <= {1, -1, -3}
        assert np.all(m1[m2 == 1] == 1) and (m2 == 1).sum() < (m1 == 1).sum()
        # the marker handed on is the one multipass hands on: C2 stays, everything else is F
        cf = np.empty_like(m2)
        cf[amg.level_perm(l)] = amg.level_cf(l)
        assert np.array_equal(cf, np.where(m2 == 1, 1, -1))
        Pref = agg2s_ref.two_stage(A, agg2s_ref.strength_rows(A, THETA), m1, m2,
                                   p12_trunc_factor=kw.get("agg_p12_trunc_factor", 0.0),
                                   p12_max=kw.get("agg_p12_max_elmts", 0),
                                   trunc_factor=kw.get("agg_trunc_factor", 0.0), pmax=kw.get("agg_pmax_elmts", 0))
        same_pattern_close_values(P, Pref)
        if kw.get("agg_pmax_elmts", 0):
            assert np.diff(P.indptr).max() <= kw["agg_pmax_elmts"]
    # levels below the aggressive ones have no stage markers
    if amg.num_levels - 1 > nagg:
        with pytest.raises(mi.HypreError):
            amg.level_agg_markers(nagg)
        mi.call("HYPRE_ClearAllErrors")


@pytest.mark.parametrize("name,kw", [("lap7_12", dict(agg_num_levels=1)), ("aniso", dict(agg_num_levels=2, agg_pmax_elmts=4)),
                                     ("randmm", dict(agg_num_levels=1, agg_p12_max_elmts=4)),
                                     ("lap27_10", dict(agg_num_levels=1, agg_trunc_factor=0.2))])
def test_properties_seen_from_outside(mi_lib, name, kw):
    mi = mi_lib
    amg = host_amg(mi, operator(mi, name), agg_interp_type=5, **kw)
    seen_zero_sum_rows = 0
    for l in range(min(kw["agg_num_levels"], amg.num_levels - 1)):
        A, P, cf = csr(amg, l, 0), csr(amg, l, 2), amg.level_cf(l)
        m1, m2 = amg.level_agg_markers(l)
        n, nc = P.shape
        assert nc == int((m2 == 1).sum()) and np.array_equal(cf == 1, m2 == 1)
        # rows of C2 points are unit rows (C-first ordering: C point q is coarse unknown q of the level's natural
        # numbering, which the next level's own C-first ordering then permutes)
        permc = amg.level_perm(l + 1)
        rows_c = np.flatnonzero(m2 == 1)
        assert np.array_equal(np.diff(P.indptr)[rows_c], np.ones(len(rows_c), dtype=int))
        assert np.array_equal(P.data[P.indptr[rows_c]], np.ones(len(rows_c)))
        assert np.array_equal(permc[P.indices[P.indptr[rows_c]]], np.arange(nc))
        # rows of special F points are empty
        assert np.all(np.diff(P.indptr)[m2 == -3] == 0)
        # rows sum to 1 wherever every row of A they depend on sums to zero: the rows within four steps of the graph
        # of A (two per stage), none of them special
        rs = np.abs(np.asarray(A.sum(axis=1)).ravel()) > 1e-12 * np.abs(A.diagonal())
        G = (abs(A) + sp.identity(n)).tocsr()
        G.data[:] = 1.0
        bad = (rs | (m2 == -3) | (m1 == -3)).astype(float)
        for _ in range(4):
            bad = G @ bad
        ok = (bad == 0) & (np.diff(P.indptr) > 0)
        seen_zero_sum_rows += int(ok.sum())
        sums = np.asarray(P.sum(axis=1)).ravel()
        assert np.all(np.abs(sums[ok] - 1.0) < 1e-12), np.abs(sums[ok] - 1.0).max()
        # Galerkin: A_c = P^T A P, in the next level's ordering
        Ac = csr(amg, l + 1, 0)
        G2 = (P.T @ A @ P).tocsr()
        assert abs(Ac - G2).max() <= 1e-12 * abs(Ac).max()
        R = csr(amg, l, 3)
        assert abs(R - P.T).nnz == 0
    if name in ("lap7_12", "aniso"):
        assert seen_zero_sum_rows > 0


def test_two_grid_factor_beats_multipass_on_the_same_splitting(mi_lib):
    """12^3, one aggressive level, the library's own splitting (the same for both: one coarsening, two interpolations).
    Measured (profiles/agg2s_two_grid.txt): 0.346 against 0.433."""
    mi = mi_lib
    A = operator(mi, "lap7_12")
    a5 = host_amg(mi, A, agg_num_levels=1, agg_interp_type=5, agg_pmax_elmts=4)
    a4 = host_amg(mi, A, agg_num_levels=1, agg_interp_type=4)
    assert np.array_equal(a5.level_cf(0), a4.level_cf(0)) and np.array_equal(a5.level_perm(0), a4.level_perm(0))
    f5 = two_grid_factor(csr(a5, 0, 0), csr(a5, 0, 2))
    f4 = two_grid_factor(csr(a4, 0, 0), csr(a4, 0, 2))
    print("two-grid factor at 12^3: two-stage extended %.4f (%.2f entries per row), multipass %.4f (%.2f)"
          % (f5, csr(a5, 0, 2).nnz / 1728.0, f4, csr(a4, 0, 2).nnz / 1728.0))
    assert f5 < f4, (f5, f4)


def test_zero_denominator_fails_setup_naming_level_and_row(mi_lib):
    """d_i = 0 with a non-empty numerator (tests/agg2s_common.py zero_denominator_matrix)."""
    mi = mi_lib
    A = ij_host(mi, zero_denominator_matrix())
    amg = mi.BoomerAMG(print_level=0, agg_num_levels=1, agg_interp_type=5)
    with pytest.raises(mi.HypreError, match=r"level 0: row \d+ has a zero denominator"):
        mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
    mi.call("HYPRE_ClearAllErrors")
    # multipass on the same matrix does not care
    host_amg(mi, A, agg_num_levels=1)


@pytest.mark.parametrize("nproc,n,seq,agg", [(2, 12, 0, 1), (3, 10, -1, 2)])
def test_replicated_setup_on_gloo_ranks_gives_the_single_rank_hierarchy(nproc, n, seq, agg):
    env = dict(os.environ, MI_HYPRE_HOST_THREADS="2", OMP_NUM_THREADS="1", MI_HYPRE_LOCALITY_ORDER="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr",
           "127.0.0.1", "--master-port", str(30911 + nproc + n), WORKER, "--mode", "host", "--grid", str(n), "--seq", str(seq),
           "--agg", str(agg)]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    assert p.stdout.count("agg2s rank ok") == nproc, p.stdout[-4000:]
