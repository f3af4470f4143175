"""The specification of unknown-based systems AMG ("Systems of PDEs") restated with numpy, level
by level: strength graph, splitting and interpolation of a level are those of the same-function operator F(A_l), the
coarse dof_func is the fine one at the C points, everything else reads the full A_l.

The reference of one level is a scalar TWO-level setup on the numpy-filtered operator: by the oracle for the settings
the oracle restates (interp_type 0 / 4 / 6, coarsen_type 8 / 6, agg_interp_type 4), by the library's own host-only
scalar setup (num_functions 1) otherwise (interp_type 17 / 100, agg_interp_type 5)."""
import numpy as np
import scipy.sparse as sp

from tests.agg2s_common import csr, ij_host
from tests.setup_reuse_ref import triple_product_scipy


def filter_same_function(A, dof):
    """F(A): the entries a_ij with dof[i] == dof[j] and the diagonal, rows in their stored order"""
    A = sp.csr_matrix(A)
    dof = np.asarray(dof)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    keep = (dof[rows] == dof[A.indices]) | (rows == A.indices)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=A.shape[0]))])
    return sp.csr_matrix((A.data[keep], A.indices[keep], indptr), shape=A.shape)


def coarse_dof_func(dof, cf):
    return np.asarray(dof)[np.asarray(cf) == 1]


def canonical(M):
    """CSR with ascending columns, explicit zeros kept"""
    M = sp.csr_matrix(M)
    M.sort_indices()
    return M


def _natural(A, P, cf, perm, permc):
    """reported (C-first) arrays -> the level's natural numbering; coarse unknown c = the c-th C point in it.  perm[new]
    = old (perm of level 0 may lead to the caller's rows: the hierarchies of these tests are built without the internal
    numbering, or the caller says what `old` means)"""
    perm, permc = np.asarray(perm, dtype=np.int64), np.asarray(permc, dtype=np.int64)
    n = len(perm)
    out = {}
    if A is not None:
        c = sp.coo_matrix(A)
        out["A"] = canonical(sp.csr_matrix((c.data, (perm[c.row], perm[c.col])), shape=A.shape))
    if P is not None:
        c = sp.coo_matrix(P)
        # (coo of a csr keeps explicit zeros)
        out["P"] = canonical(sp.csr_matrix((c.data, (perm[c.row], permc[c.col])), shape=P.shape))
    if cf is not None:
        m = np.empty(n, dtype=np.int64)
        m[perm] = cf
        out["cf"] = m
    return out


def product_levels(amg, with_dof=True, order0=None):
    """every level of a product hierarchy in its natural numbering: dicts with A, and P, R, cf below the coarsest; dof
    when the hierarchy keeps one.  order0: what level 0's natural numbering means when the internal locality numbering
    was applied (level_perm(0) leads to caller rows: position of caller row r in the internal numbering)"""
    out = []
    nlev = amg.num_levels
    for l in range(nlev):
        perm = amg.level_perm(l).astype(np.int64)
        if l == 0 and order0 is not None:
            perm = np.asarray(order0)[perm]
        last = l == nlev - 1
        permc = None if last else amg.level_perm(l + 1).astype(np.int64)
        d = _natural(csr(amg, l, 0), None if last else csr(amg, l, 2), None if last else amg.level_cf(l), perm,
                     perm if last else permc)
        if not last:
            R = sp.coo_matrix(csr(amg, l, 3))
            d["R"] = canonical(sp.csr_matrix((R.data, (permc[R.row], perm[R.col])), shape=R.shape))
        if with_dof:
            dof = np.empty(len(perm), dtype=np.int64)
            dof[perm] = amg.level_dof_func(l)
            d["dof"] = dof
        out.append(d)
    return out


ORACLE_KEYS = {"interp_type": "interp_type", "coarsen_type": "coarsen_type", "true_pmax_elmts": "pmax_elmts",
               "agg_num_levels": "agg_num_levels", "agg_interp_type": "agg_interp_type", "strong_threshold": "strong_threshold"}


def oracle_restates(kw):
    return kw.get("interp_type", 6) in (0, 4, 6) and kw.get("agg_interp_type", 4) == 4


def two_level_reference(mi, oc, F, kw, aggressive):
    """(cf, P) of a scalar two-level setup on F in F's numbering, or None when that setup does not coarsen.  kw: the
    BoomerAMG keyword arguments of the hierarchy under test (num_functions / dof_func are not handed on);
    aggressive: whether the level is an aggressive one there"""
    kw = {k: v for k, v in kw.items() if k not in ("num_functions", "dof_func")}
    kw["agg_num_levels"] = 1 if aggressive else 0
    if oracle_restates(kw):
        par = {ORACLE_KEYS[k]: v for k, v in kw.items()}
        par.setdefault("pmax_elmts", 0)
        o = oc.Amg(oc.Csr.from_scipy(F), oc.default_params(max_levels=2, coarsen_type=par.pop("coarsen_type", 8), **par))
        if o.num_levels < 2:
            return None
        d = _natural(None, o.level_P(0).to_scipy(), o.level_cf(0), o.level_perm(0), o.level_perm(1))
    else:
        a = mi.BoomerAMG(print_level=0, max_levels=2, **kw)
        Fij = ij_host(mi, F)  # (alive until the setup has returned)
        mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", a.h, Fij.par)
        if a.num_levels < 2:
            return None
        d = _natural(None, csr(a, 0, 2), a.level_cf(0), a.level_perm(0), a.level_perm(1))
    return d["cf"], d["P"]


def same_bits(X, Y):
    X, Y = canonical(X), canonical(Y)
    return (X.shape == Y.shape and np.array_equal(X.indptr, Y.indptr) and np.array_equal(X.indices, Y.indices)
            and np.array_equal(X.data, Y.data))


def check_hierarchy(mi, oc, amg, A0, dof0, kw):
    """every statement of the specification, on every level of a host-only hierarchy built from (A0, dof0) under kw;
    returns the number of levels checked"""
    lev = product_levels(amg)
    assert same_bits(lev[0]["A"], A0) and np.array_equal(lev[0]["dof"], dof0)
    for l, d in enumerate(lev[:-1]):
        A, dof, nxt = d["A"], d["dof"], lev[l + 1]
        F = filter_same_function(A, dof)
        ref = two_level_reference(mi, oc, F, kw, aggressive=l < kw.get("agg_num_levels", 0))
        assert ref is not None, "the reference does not coarsen level %d" % l
        cf_ref, P_ref = ref
        assert np.array_equal(d["cf"], cf_ref), "cf of level %d" % l
        assert same_bits(d["P"], P_ref), "P of level %d" % l
        assert same_bits(d["R"], d["P"].T), "R of level %d" % l
        # the coarse operator reads the FULL A
        # (tests/test_setup_reuse_spec.py's bound for this comparison: 1e-13 (|P^T| |A| |P|)_ij, same stored pattern)
        C, B = triple_product_scipy(A, d["P"])
        got = nxt["A"]
        # scipy drops the entries whose products cancel exactly (the mixed derivatives of the Lame operator do) or
        # multiply stored zeros; the library stores them: the stored pattern is the structural one, and where C or B
        # have no entry they count as 0 (so a stored entry with B_ij = 0 must be exactly 0)
        ones = lambda X: sp.csr_matrix((np.ones(X.nnz), X.indices, X.indptr), shape=X.shape)
        pat = canonical(ones(d["P"]).T @ (ones(A) @ ones(d["P"])))
        assert np.array_equal(pat.indptr, got.indptr) and np.array_equal(pat.indices, got.indices), l
        diff = abs(got - C).tocsr()
        slack = (1e-13 * B - diff).tocsr()
        over = diff.multiply(B.power(-1.0)).tocsr()  # (on B's pattern)
        ratio = over.max() if over.nnz else 0.0
        print("level %d: n %d -> %d, max |A_c - P^T A P| / (|P^T| |A| |P|) = %.3e" % (l, A.shape[0], C.shape[0], ratio))
        assert slack.nnz == 0 or slack.data.min() >= 0.0, (l, ratio)
        assert np.array_equal(nxt["dof"], coarse_dof_func(dof, d["cf"])), "dof_func of level %d" % (l + 1)
        Pc = sp.coo_matrix(d["P"])
        assert np.array_equal(dof[Pc.row], nxt["dof"][Pc.col]), "P of level %d links different functions" % l
    return len(lev) - 1
