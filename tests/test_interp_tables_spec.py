"""CPU: the operators of tests/test_gpu_interp_tables.py (tests/systems.py: INTERP_TABLE_OPERATORS) and what they make the
device interpolation kernel run.  sk::interp sorts the rows of a level by a bound T on their interpolatory set and runs
one instantiation of interp_group_k per bin (tables of 16, 32, 32-then-128, 512 and 1024 entries; one row over 1024
sends the level to the host routine).  This module states the bound and the truncation rule a second time in plain
Python, asserts from the matrix, the strength rows and the oracle's marks alone that the operators reach every table,
fill it to its capacity and to one more, with negative diagonals, special F points, zero distribution sums and ties in
|weight|, and holds the oracle on these long rows against the formulas of tests/interp_ref.py and the library's host
setup against the oracle."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.agg2s_ref import strength_rows
from tests.interp_ref import classical_modified_reference, extended_i_reference, strength_pattern
from tests.systems import INTERP_TABLE_OPERATORS, HUB_EXT_LENGTHS, HUB_LENGTHS, interp_table_operator
from tests.test_mixed_sign_spec import assert_levels_equal, host_setup, library_levels, oracle_levels

CENSUS_KEYS = ("cap16", "cap32", "try32_kept", "try32_retried", "cap512", "cap1024")


# ---------------------------------------------------------------------------------------------------------------
# the bound and its bins, from the rule stated at interp_bound_k
# ---------------------------------------------------------------------------------------------------------------
def interp_bounds(strong, cf, ext):
    """(T, distinct, nstrong) per row, all zero for rows that are not F points with a strong connection.
    trc = the strong C neighbours of the row plus, for ext+i, the strong C neighbours of each of its strong F
    neighbours -- counted every time they are met; T = max(trc, number of strong connections).  distinct = the size of
    the interpolatory set itself.  The marks are the ones the interpolation starts from: a special F point (-3 then,
    -1 afterwards) has no strong connection, so it has T = 0 itself and adds nothing to a neighbour's count -- the
    marks after -3 -> -1 give the same numbers."""
    n = len(strong)
    cf = np.asarray(cf)
    T, distinct, nstrong = (np.zeros(n, dtype=np.int64) for _ in range(3))
    cs = [[j for j in s if cf[j] == 1] for s in strong]
    for i in range(n):
        if cf[i] == 1 or len(strong[i]) == 0:
            continue
        cand = list(cs[i])
        if ext:
            for k in strong[i]:
                if cf[k] != 1:
                    cand += cs[k]
        T[i] = max(len(cand), len(strong[i]))
        distinct[i] = len(set(cand))
        nstrong[i] = len(strong[i])
    return T, distinct, nstrong


def predicted_census(T, distinct, nstrong):
    """What HYPRE_MI_BoomerAMGGetInterpCensus must report for rows with these numbers: a row goes to the smallest table
    that holds T; rows with 33 <= T <= 128 are first tried in 32-entry tables, which a row keeps iff its distinct
    candidates and its strong connections both fit in 32; a single T over 1024 and nothing runs."""
    out = dict.fromkeys(CENSUS_KEYS, 0)
    out.update(max_bound=int(T.max()), fell_back=bool(T.max() > 1024), host=False)
    if out["fell_back"]:
        return out
    mid = (T > 32) & (T <= 128)
    fits = (distinct <= 32) & (nstrong <= 32)
    out.update(cap16=int((T <= 16).sum()), cap32=int(((T > 16) & (T <= 32)).sum()), try32_kept=int((mid & fits).sum()),
               try32_retried=int((mid & ~fits).sum()), cap512=int(((T > 128) & (T <= 512)).sum()),
               cap1024=int(((T > 512) & (T <= 1024)).sum()))
    return out


def discovery_order(strong, cf, i, ext):
    """the interpolatory set of row i (fine ids) in the order the row's walk meets it: the strong connections in stored
    order, a C point itself, a strong F neighbour (ext+i) through the C points of its own strong row in stored order"""
    seen, out = set(), []
    for k in strong[i]:
        for j in ([k] if cf[k] == 1 else [j for j in strong[k] if cf[j] == 1] if ext else []):
            if j not in seen:
                seen.add(j)
                out.append(j)
    return out


def truncate_row(vals, factor, pmax):
    """vals in discovery order -> ({position: new value}, tie-break decisions).  Keep the entries >= factor * max |p|;
    of those the pmax largest by |p| descending, then position ascending; rescale the kept ones to the row sum."""
    big = max(abs(v) for v in vals)
    keep = [q for q, v in enumerate(vals) if factor <= 0.0 or abs(v) >= factor * big]
    ties = 0
    if pmax > 0 and len(keep) > pmax:
        ranked = sorted(keep, key=lambda q: (-abs(vals[q]), q))
        ties = int(abs(vals[ranked[pmax - 1]]) == abs(vals[ranked[pmax]]))  # last kept and first dropped tie in |p|
        keep = sorted(ranked[:pmax])
    total = kept = 0.0
    for v in vals:
        total += v
    for q in keep:
        kept += vals[q]
    scale = total / kept if kept != 0.0 else 1.0
    return {q: vals[q] * scale for q in keep}, ties


# ---------------------------------------------------------------------------------------------------------------
# per operator, built once: the level-0 facts in the NATURAL numbering, which is the one the device kernel works in
# (the hierarchies report every level C points first; counts do not depend on the numbering, discovery order does)
# ---------------------------------------------------------------------------------------------------------------
_state = {}


def oracle_params(oc, name, kw, **more):
    """the oracle's parameters for library keywords kw on the operator `name`"""
    okw = {("pmax_elmts" if k == "true_pmax_elmts" else k): v for k, v in library_kw(name, kw).items()}
    return oc.default_params(**okw, **more)


def library_kw(name, kw):
    return dict(dict(strong_threshold=INTERP_TABLE_OPERATORS[name][1]), **kw)


def state(oc, name):
    """dict: M, hubs, lengths, theta, strong (rows of the strength graph), cf (natural numbering), perm0"""
    if name not in _state:
        M, hubs, lengths = interp_table_operator(name)
        theta = INTERP_TABLE_OPERATORS[name][1]
        amg = oc.Amg(oc.Csr.from_scipy(M), oc.default_params(strong_threshold=theta))
        perm0 = np.asarray(amg.level_perm(0))
        cf = np.zeros(M.shape[0], dtype=np.int64)
        cf[perm0] = np.asarray(amg.level_cf(0))  # (the splitting depends on the strength graph alone)
        A0 = amg.level_A(0).to_scipy().tocsr()
        assert abs(A0 - M[perm0][:, perm0]).max() == 0.0
        _state[name] = dict(M=M, hubs=hubs, lengths=lengths, theta=theta, strong=strength_rows(M, theta, 0.9), cf=cf, bounds={})
    return _state[name]


def bounds(oc, name, interp):
    st = state(oc, name)
    if interp not in st["bounds"]:
        st["bounds"][interp] = interp_bounds(st["strong"], st["cf"], interp == 6)
    return st["bounds"][interp]


def oracle_P_natural(amg):
    """level-0 P of an oracle hierarchy with rows in the natural numbering and column c = the c-th C point in it"""
    P = amg.level_P(0).to_scipy().tocoo()
    perm0, perm1 = np.asarray(amg.level_perm(0)), np.asarray(amg.level_perm(1))
    return sp.csr_matrix((P.data, (perm0[P.row], perm1[P.col])), shape=P.shape)


_refs = {}


def reference_P(oc, name, interp):
    """untruncated level-0 P by the formulas of tests/interp_ref.py, natural numbering; computed once, not modified"""
    if (name, interp) not in _refs:
        st = state(oc, name)
        S = strength_pattern(st["M"], st["theta"], 0.9)
        ref = extended_i_reference if interp == 6 else classical_modified_reference
        _refs[name, interp] = ref(st["M"], S, st["cf"]).tocsr()
    return _refs[name, interp]


# ---------------------------------------------------------------------------------------------------------------
# conditions
# ---------------------------------------------------------------------------------------------------------------
def test_hubs_fill_every_table_to_its_capacity_and_one_more(oc):
    """classical interpolation on `hubs`: every planted length is an F row whose bound is exactly that length -- 16 / 17,
    32 / 33, 128 / 129, 512 / 513 and 1024 -- in each of the four styles, with hundreds of distinct C points in the
    long ones; no other row is long"""
    st = state(oc, "hubs")
    T, distinct, nstrong = bounds(oc, "hubs", 0)
    hubs, lengths = st["hubs"], st["lengths"]
    assert sorted(set(lengths)) == sorted(HUB_LENGTHS) and len(hubs) == 4 * len(HUB_LENGTHS)
    assert np.all(st["cf"][hubs] == -1)
    assert np.array_equal(T[hubs], lengths) and np.array_equal(nstrong[hubs], lengths)
    d = st["M"].diagonal()
    for L in HUB_LENGTHS:
        rows = hubs[lengths == L]
        assert len(rows) == 4 and (d[rows] > 0).sum() == 2 and (d[rows] < 0).sum() == 2
        assert np.all(distinct[rows] >= (5 if L <= 33 else 30 if L <= 129 else 140 if L <= 513 else 300)), (L, distinct[rows])
    rest = np.delete(T, hubs)
    assert rest.max() <= 32
    print("hubs, classical: distinct C points of the hubs", dict(zip(lengths.tolist(), distinct[hubs].tolist())))


def test_hubs_ext_straddle_the_table_sizes(oc):
    """ext+i on `hubs_ext`: bounds within 8 below and within 8 above 128 and 512 (128, 129, 512 and 513 themselves are
    there), every row at most 1024, and rows in each of the tables of 128, 512 and 1024 entries"""
    st = state(oc, "hubs_ext")
    T, distinct, nstrong = bounds(oc, "hubs_ext", 6)
    assert len(st["hubs"]) == len(HUB_EXT_LENGTHS) and np.all(st["cf"][st["hubs"]] == -1)
    for cap in (128, 512):
        assert ((T > cap - 8) & (T <= cap)).any() and ((T > cap) & (T <= cap + 8)).any(), cap
    for exact in (128, 129, 512, 513):
        assert (T == exact).any(), exact
    assert 900 < T.max() <= 1024
    want = predicted_census(T, distinct, nstrong)
    print("hubs_ext, ext+i:", want)
    assert min(want[k] for k in ("try32_retried", "cap512", "cap1024")) >= 5
    # the same operator under classical interpolation stays in the tables up to 1024 as well
    assert bounds(oc, "hubs_ext", 0)[0].max() == max(HUB_EXT_LENGTHS)


def _sign_exposed(st, T, lo, hi):
    """rows with lo < T <= hi that have a negative diagonal or a strong F neighbour with a negative diagonal"""
    d, cf, strong = st["M"].diagonal(), st["cf"], st["strong"]
    return sum(1 for i in np.flatnonzero((T > lo) & (T <= hi)) if d[i] < 0 or any(cf[k] != 1 and d[k] < 0 for k in strong[i]))


def test_long_rows_meet_every_branch(oc):
    """over all operators in the setting they were made for: at least 100 rows in the 512-entry tables and 20 rows in the
    1024-entry tables with a negative diagonal or a negative-diagonal strong F neighbour (the dense operators alone
    give that); and among the rows with T > 128 at least one special F neighbour and one strong F neighbour with a
    zero distribution sum, counted by the formulas of tests/interp_ref.py on those rows alone"""
    exposed = {}
    for name in ("dense1200", "dense1600", "hubs", "hubs_ext"):
        interp = INTERP_TABLE_OPERATORS[name][2]
        T = bounds(oc, name, interp)[0]
        exposed[name] = (_sign_exposed(state(oc, name), T, 128, 512), _sign_exposed(state(oc, name), T, 512, 1024))
    print("rows exposed to a negative diagonal (T 129..512, T 513..1024):", exposed)
    assert exposed["dense1200"][0] >= 100 and exposed["dense1600"][0] >= 100
    assert exposed["dense1600"][1] >= 20
    assert exposed["hubs"][0] >= 8 and exposed["hubs"][1] >= 8 and min(exposed["hubs_ext"]) >= 5
    events = {}
    for name, interp in (("hubs", 0), ("hubs_ext", 6), ("hubs_ext", 0)):
        st = state(oc, name)
        T = bounds(oc, name, interp)[0]
        census = {}
        ref = extended_i_reference if interp == 6 else classical_modified_reference
        ref(st["M"], strength_pattern(st["M"], st["theta"], 0.9), st["cf"], census, only_rows=set(np.flatnonzero(T > 128)))
        events[name, interp] = census
        assert census["special_f"] >= 1, (name, interp, census)
    print("special F neighbours / zero-sum neighbours of the rows with T > 128:", events)
    assert events["hubs", 0]["zero_sum"] >= 1 and events["hubs_ext", 0]["zero_sum"] >= 1
    assert sum(c["zero_sum"] for c in events.values()) >= 1


@pytest.mark.parametrize("name", ["overflow", "overflow_ext"])
def test_overflow_operators_have_exactly_one_row_over_the_largest_table(oc, name):
    st = state(oc, name)
    interp = INTERP_TABLE_OPERATORS[name][2]
    T = bounds(oc, name, interp)[0]
    over = np.flatnonzero(T > 1024)
    assert list(over) == [st["hubs"][-1]] and st["lengths"][-1] == (1025 if interp == 0 else 560)
    assert 1024 < T[over[0]] <= 1040
    assert predicted_census(*bounds(oc, name, interp))["fell_back"]


# ---------------------------------------------------------------------------------------------------------------
# the oracle against the formulas, untruncated and truncated
# ---------------------------------------------------------------------------------------------------------------
FORMULA_CASES = [("hubs", 0), ("hubs", 6), ("hubs_ext", 6), ("hubs_ext", 0), ("dense1200", 6), ("dense1200", 0)]
FORMULA_BAR = 9e-15


@pytest.mark.parametrize("name,interp", FORMULA_CASES)
def test_oracle_matches_the_formulas_on_long_rows(oc, name, interp):
    """Level-0 P without truncation against tests/interp_ref.py: rows of up to 1024 strong connections, 750 entries and
    (hubs under ext+i) 1974 candidates.  Measured max |P_oracle - P_formula|: hubs 7.77e-16 (classical) and 1.39e-16
    (ext+i), hubs_ext 9.99e-16 and 1.67e-16, dense1200 3.33e-16 and 6.94e-17.  The bar is 9e-15, below ten times the
    worst of them (the short rows of tests/test_mixed_sign_spec.py have 1e-13)."""
    st = state(oc, name)
    Pref = reference_P(oc, name, interp)
    amg = oc.Amg(oc.Csr.from_scipy(st["M"]), oracle_params(oc, name, dict(interp_type=interp, true_pmax_elmts=0)))
    Po = oracle_P_natural(amg)
    assert Po.shape == Pref.shape
    err = abs(Po - Pref).max()
    longest = int(np.diff(Po.indptr).max())
    print("%s interp %d: max |P_oracle - P_formula| = %.2e, longest row of P %d" % (name, interp, err, longest))
    assert err < FORMULA_BAR
    assert longest == bounds(oc, name, interp)[1].max()  # (the whole interpolatory set of the longest row is there)


TRUNCATIONS = [dict(true_pmax_elmts=4), dict(true_pmax_elmts=2, trunc_factor=0.2), dict(true_pmax_elmts=0, trunc_factor=0.2)]


def test_oracle_truncation_matches_the_rule_and_position_breaks_ties(oc):
    """the truncation rule applied to the formulas' rows against the oracle's truncated P (pmax 4; pmax 2 with factor
    0.2; factor 0.2 alone), same bar (9.99e-16 measured); and in rows with T > 128 the choice between the last kept and
    the first dropped entry is made by position alone (equal |p|) at least once (40 times, measured)"""
    tie_rows = 0
    for name, interp in FORMULA_CASES:
        st = state(oc, name)
        Pref = reference_P(oc, name, interp)
        T = bounds(oc, name, interp)[0]
        cidx = np.cumsum(st["cf"] == 1) - 1
        frows = np.flatnonzero(T > 0)
        order = {i: discovery_order(st["strong"], st["cf"], i, interp == 6) for i in frows}
        for kw in TRUNCATIONS:
            amg = oc.Amg(oc.Csr.from_scipy(st["M"]), oracle_params(oc, name, dict(kw, interp_type=interp)))
            Po = oracle_P_natural(amg)
            worst = 0.0
            for i in frows:
                vals = [Pref[i, cidx[j]] for j in order[i]]
                if not vals:
                    assert Po.indptr[i + 1] == Po.indptr[i]
                    continue
                kept, ties = truncate_row(vals, kw.get("trunc_factor", 0.0), kw["true_pmax_elmts"])
                tie_rows += int(ties and T[i] > 128)
                want = sorted((cidx[order[i][q]], v) for q, v in kept.items())
                got_c = Po.indices[Po.indptr[i]:Po.indptr[i + 1]]
                got_v = Po.data[Po.indptr[i]:Po.indptr[i + 1]]
                o = np.argsort(got_c)
                assert [c for c, _ in want] == list(got_c[o]), (name, interp, kw, i)
                worst = max(worst, max(abs(v - g) for (_, v), g in zip(want, got_v[o])))
            print("%s interp %d %s: max |P_oracle - truncated formula| = %.2e" % (name, interp, kw, worst))
            assert worst < FORMULA_BAR, (name, interp, kw)
    print("rows with T > 128 whose truncation is decided by position:", tie_rows)
    assert tie_rows >= 1


# ---------------------------------------------------------------------------------------------------------------
# the library's host setup
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(INTERP_TABLE_OPERATORS))
def test_host_setup_equals_oracle(mi_lib, oc, name):
    """every level of the host-only setup equals the oracle's bit for bit, with the interpolation the operator was made
    for, untruncated and with the default pmax 4"""
    M = interp_table_operator(name)[0]
    for kw in (dict(true_pmax_elmts=0), {}):
        kw = dict(kw, interp_type=INTERP_TABLE_OPERATORS[name][2])
        amg = host_setup(mi_lib, M, library_kw(name, kw))
        for l in range(amg.num_levels):  # (the device kernel was not asked: zeros and the host flag)
            assert amg.interp_census(l) == dict(dict.fromkeys(CENSUS_KEYS, 0), max_bound=0, fell_back=False, host=True)
        lib = library_levels(amg)
        want = oracle_levels(oc.Amg(oc.Csr.from_scipy(M), oracle_params(oc, name, kw)))
        assert len(want) >= 3
        assert_levels_equal(lib, want)
