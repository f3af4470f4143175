"""GPU: the value-dictionary instantiations -- spmv_stream_xc<*, *, true, 256>, spmv_stream_xc<*, 0, true, 512>,
gs_tile_k<true, 256>, gs_tile_k<true, 512> -- on operators other than the constant-coefficient stencil.

Every operator of tests/dict_cases.py is placed twice, with the dictionary on and off (HYPRE_MI_SetValueDictionary:
process-wide, read when an operator is put into the solve format).  The two must give the same bits: the table holds
the very doubles of the plain stream, and both kernels form and add the products in the same order.  One of them is
also held against a reference: SpMV against a long double product, by the bound of a dot product in any summation
order (dict_cases.reference_matvec); relaxation against the oracle, 1e-12 relative to max|u| as everywhere in this
suite.  Which kernel ran is read from the value kind of the operator and from the instantiation name that the launch
leaves in its profile class; the launch geometry (lanes per row, unique columns per tile, rows longer than a tile) from
the operator the library reports back, by the rules restated in dict_cases.tile_schedule, whose tile count is checked
against the census of the library's own schedule.  tests/test_value_dictionary_spec.py checks the generators."""
import numpy as np
import pytest

from tests import dict_cases as dc

pytestmark = pytest.mark.gpu

TOL = 1e-12
GS_TYPES = [3, 4, 6, 8, 13, 14]
JACOBI_TYPES = [7, 18]


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def first_difference(a, b):
    d = np.flatnonzero(np.asarray(a).view(np.int64) != np.asarray(b).view(np.int64))
    return None if len(d) == 0 else (int(d[0]), float(a[d[0]]), float(b[d[0]]), len(d))


@pytest.fixture
def dictionary(mi):
    """switch(on) for the operators placed next; on again afterwards, whatever happened"""
    try:
        yield mi.set_value_dictionary
    finally:
        mi.set_value_dictionary(True)


@pytest.fixture
def kernel_names(mi):
    """name(pid): the instantiation last launched under a profile class; the classes are switched off again afterwards"""
    pids = (mi.PROF_SPMV_L0, mi.PROF_LVL_RELAX, mi.PROF_LVL_RELAX + 1, mi.PROF_LVL_RELAX0)  # (per level: 0, 1, 0)
    for pid in pids:
        mi.profile_enable(pid, 8)
    try:
        yield mi.profile_kernel_name
    finally:
        for pid in pids:
            mi.profile_enable(pid, 0)


@pytest.fixture
def zero_guess_mode(mi):
    """set(mode) for the hierarchies set up next (1: the level operator with zero_from, 3: the sub-operators)"""
    try:
        yield lambda mode: mi.call("HYPRE_MI_SetZeroGuessMode", mode)
    finally:
        mi.call("HYPRE_MI_SetZeroGuessMode", 3)


def _chunk(mi):
    c = mi.c_int()
    mi.call("HYPRE_MI_GetGSChunk", mi.C.byref(c))
    return c.value


def _width(M):
    return 512 if M.nnz / M.shape[0] >= 100.0 else 256


# ---------------------------------------------------------------- SpMV
_ratios = {}


@pytest.mark.parametrize("name", list(dc.SPMV) + list(dc.GIANT) + list(dc.REFUSALS))
def test_spmv_on_off_and_against_long_double(mi, dictionary, kernel_names, name):
    M, info = dc.spmv_case(name)
    n, w = M.shape[0], _width(M)
    mats = {}
    for on in (True, False):
        dictionary(on)
        mats[on] = mi.matrix_from_scipy(M)
    dictionary(True)
    assert mi.parcsr_value_kind(mats[True]) == info["kind"] and mi.parcsr_value_kind(mats[False]) == 0
    # the device block holds the generator's entries at the generator's positions ...
    ia, ja, a, shape = mi.parcsr_csr(mats[True], 2)
    assert shape == M.shape and np.array_equal(ia, M.indptr) and np.array_equal(ja, M.indices) and same(a, M.data)
    h = mi.parcsr_csr(mats[True], 0)
    assert np.array_equal(h[0], ia) and np.array_equal(h[1], ja) and same(h[2], a)
    # ... so what decides the case is where the sample of k::build_value_dictionary does or does not look
    nnz, L = len(a), np.diff(ia)
    pos = dc.sample_positions(nnz)
    seen = len(np.unique(dc.bits(a[pos])))
    if name == "distinct257":
        assert seen == 257 and nnz // dc.THRESHOLD == 1
    elif name in ("tail_miss", "stride_miss"):
        at = np.flatnonzero(a == info["extra"])
        assert len(at) >= 2 and not np.isin(at, pos).any() and seen == 20 and len(np.unique(dc.bits(a))) == 21
        assert (at.min() >= dc.THRESHOLD and nnz // dc.THRESHOLD == 1) if name == "tail_miss" else \
            (np.all(at % 2 == 1) and at.min() < dc.THRESHOLD and nnz // dc.THRESHOLD == 2)
    elif name in ("below_threshold", "at_threshold"):
        assert nnz == dc.THRESHOLD - (name == "below_threshold") and seen <= 256
    else:
        table = np.sort(np.unique(dc.bits(a)))
        assert len(table) == dc.distinct(M) <= 256
        idx = np.searchsorted(table, dc.bits(a))
        if name in ("distinct256", "wide", "giant-wide"):
            assert len(table) == 256
            assert (idx[0::2] == 255).any() and (idx[1::2] == 255).any()  # low and high byte of a loaded index pair
        assert idx.max() > 2 and (a[idx == idx.max()] > 0).all() and (a[idx == 0] < 0).all()
    if name in dc.GIANT:
        assert L.max() == info["giant"] > 8 * w
    if name in ("ragged", "giant-ragged") or name in dc.REFUSALS:
        assert (L == 0).any()
    rng = np.random.default_rng(len(name) + n)
    xv, bv = rng.standard_normal(n), rng.standard_normal(n)
    x = mi.IJVector(0, n - 1, xv)
    worst = 0.0
    for alpha, beta in ((1.0, 0.0), (-1.5, 0.75)):
        ref, bound = dc.reference_matvec(M, xv, alpha, beta, bv)
        got = {}
        for on in (True, False):
            y = mi.IJVector(0, n - 1, bv)
            mi.call("HYPRE_ParCSRMatrixMatvec", alpha, mats[on].par, x.par, beta, y.par)
            got[on] = y.get()
            kname = kernel_names(mi.PROF_SPMV_L0)
            flag = "true" if (on and info["kind"] == 8) else "false"
            assert kname == ("spmv_stream_xc<0, 0, %s, 512>" if w == 512 else "spmv_stream_xc<0, 1, %s, 256>") % flag, kname
            err = np.abs(got[on].astype(np.longdouble) - ref)
            ratio = float(np.max(err[bound > 0] / bound[bound > 0]))
            worst = max(worst, ratio)
            print(f"{name} alpha {alpha} beta {beta} dictionary {'on' if on else 'off'} ({kname}): largest error / bound "
                  f"{ratio:.3f}, largest error {float(err.max()):.3e}")
            assert np.all(err <= bound), (name, alpha, beta, on, int(np.argmax(err - bound)))
        assert same(got[True], got[False]), (name, alpha, beta, first_difference(got[True], got[False]))
    _ratios[name] = worst
    print(f"largest SpMV error / bound so far: {max(_ratios.values()):.3f} ({max(_ratios, key=_ratios.get)})")
    for A in mats.values():
        A.destroy()


# ---------------------------------------------------------------- relaxation
def _amg(mi, M, **kw):
    A = mi.matrix_from_scipy(M)
    amg = mi.BoomerAMG(print_level=0, **kw)
    amg.setup(A)
    return A, amg


def _pair(mi, oc, dictionary, M, oracle_matrix=None, **kw):
    """hierarchies of M with the dictionary on and off, and the oracle's (of oracle_matrix when given)"""
    dictionary(True)
    on = _amg(mi, M, **kw)
    dictionary(False)
    off = _amg(mi, M, **kw)
    dictionary(True)
    okw = {k: v for k, v in kw.items() if not k.startswith("mi_")}
    oamg = oc.Amg(oc.Csr.from_scipy(M if oracle_matrix is None else oracle_matrix), oc.default_params(gs_chunk=_chunk(mi), **okw))
    for A, amg in (on, off):
        assert amg.num_levels == oamg.num_levels and amg.num_levels > 1
        assert np.array_equal(amg.level_cf(0), oamg.level_cf(0)) and np.array_equal(amg.level_perm(0), oamg.level_perm(0))
    return on, off, oamg


def _level0(amg):
    import scipy.sparse as sp

    ia, ja, a, shape = amg.level_csr(0, 0)
    return sp.csr_matrix((a, ja, ia), shape=shape)


def _check_geometry(kind, amg, A0):
    """the tiles of level 0 as the library schedules them (their count: the census), and what the case is named after"""
    t = dc.tile_census(A0)
    assert t["block"] == _width(A0) and t["entries"].max() < t["tile"]
    c = amg.gs_sweep_paths(0, 0)
    assert c is not None, "the sweep must run on the tile kernel"
    assert c["waves"] == len(t["rows"]) * (t["block"] // 64), (c, len(t["rows"]))
    assert c["general"] > 0  # (and chunks on the diagonal path: the rowlen kinds below)
    table = np.sort(np.unique(dc.bits(A0.data)))
    assert 2 < len(table) <= 256
    if kind in dc.LPR:
        assert (t["lpr"] == dc.LPR[kind]).sum() >= 10
        assert c["diagonal"] > c["general"] > 0
    if kind == "wide":
        assert np.all(t["lpr"] == 8)
    if kind == "scattered":
        assert (t["unique"] > 1024).sum() >= 0.9 * len(t["unique"])  # more than 4 * BLOCK: the second gather batch
    if kind == "ragged":
        assert len(np.unique(A0.indptr[t["rb"][:-1]] % 2)) == 2  # tile bases on odd and even stored positions
    return t


def _check_relax(mi, names, on, off, oamg, rtypes, seed, w, points_list=(0, 1, -1), off_name=None, level=0):
    """relaxation passes of `level` of the two hierarchies against level 0 of the oracle hierarchy given"""
    n = oamg.level_A(0).shape[0]
    rng = np.random.default_rng(seed)
    cf = oamg.level_cf(0)
    pid = mi.PROF_LVL_RELAX + level
    for rtype in rtypes:
        f, u0 = rng.standard_normal(n), rng.standard_normal(n)
        for points in points_list:
            got = on.relax_level(level, rtype, points, f, u0)
            name_on = names(pid)
            other = off.relax_level(level, rtype, points, f, u0)
            name_off = names(pid)
            ref = oamg.relax(0, rtype, points, f, u0)
            err = np.abs(got - ref).max()
            print(f"type {rtype} points {points}: max err {err:.3e} (max|ref| {np.abs(ref).max():.3e}) {name_on} / {name_off}")
            if rtype in GS_TYPES:
                want_on, want_off = "gs_tile_k<true, %d>" % w, off_name or "gs_tile_k<false, %d>" % w
            elif rtype in JACOBI_TYPES:
                want_on = "spmv_stream_xc<1, 0, true, %d>" % w
                want_off = ("spmv_stream_xc<1, 0, false, %d" % w) + (", true>" if off_name and off_name.endswith(", true>") else ">")
            else:  # 11: the residual SpMV of the level operator
                want_on = "spmv_stream_xc<0, 0, true, %d>" % w
                want_off = ("spmv_stream_xc<0, 0, false, %d" % w) + (", true>" if off_name and off_name.endswith(", true>") else ">")
            assert name_on == want_on and name_off == want_off, (name_on, name_off)
            assert err <= TOL * max(1.0, np.abs(ref).max())
            assert same(got, other), (rtype, points, name_on, name_off, first_difference(got, other))
            if points != 0:
                assert same(got[cf != points], u0[cf != points])


@pytest.mark.parametrize("name", list(dc.RELAX))
def test_relaxation_on_off_and_against_oracle(mi, oc, dictionary, kernel_names, name):
    kind = dc.RELAX[name][0]
    M = dc.relax_case(name)
    (A1, on), (A0_, off), oamg = _pair(mi, oc, dictionary, M)
    assert on.level_value_storage(0, 0)[0] == 8 and off.level_value_storage(0, 0)[0] == 0
    L0 = _level0(on)
    assert same(np.sort(L0.data), np.sort(M.data)) and same(_level0(off).data, L0.data)
    _check_geometry(kind, on, L0)
    for points in (0, 1, -1):
        assert on.gs_sweep_paths(0, points) is not None and off.gs_sweep_paths(0, points) is not None
    _check_relax(mi, kernel_names, on, off, oamg, GS_TYPES + JACOBI_TYPES, 900 + len(name), _width(M))


def _check_zero_pair(mi, names, on, off, oamg, seed, want_on=None):
    n = oamg.level_A(0).shape[0]
    rng = np.random.default_rng(seed)
    for rtype in GS_TYPES:
        f = rng.standard_normal(n)
        got = on.relax_pair_level(0, rtype, 1, f)
        name_on = names(mi.PROF_LVL_RELAX0)
        other = off.relax_pair_level(0, rtype, 1, f)
        name_off = names(mi.PROF_LVL_RELAX0)
        ref = oamg.relax(0, rtype, -1, f, oamg.relax(0, rtype, 1, f, np.zeros(n)))
        err = np.abs(got - ref).max()
        print(f"type {rtype} zero-guess C-then-F: max err {err:.3e} (max|ref| {np.abs(ref).max():.3e}) {name_on} / {name_off}")
        if want_on:
            assert name_on == want_on and name_off == want_on.replace("true", "false"), (name_on, name_off)
        assert err <= TOL * max(1.0, np.abs(ref).max())
        assert same(got, other), (rtype, name_on, name_off, first_difference(got, other))


@pytest.mark.parametrize("mode", [1, 3])
@pytest.mark.parametrize("name", list(dc.ZERO))
def test_zero_guess_pairs_on_off_and_against_oracle(mi, oc, dictionary, kernel_names, zero_guess_mode, name, mode):
    """C pass then F pass from u = 0.  Mode 1 sweeps the level operator and is told where the zeros start; mode 3 sweeps
    the zero-guess sub-operator, which has a dictionary of its own where it has an x cache and 65536 entries -- `ragged`
    at 16 001 rows; the sub-operators of the rowlen kinds have 2.4 entries per row at any size and never get one."""
    zero_guess_mode(mode)
    kind = dc.ZERO[name][0]
    M = dc.relax_case(name)
    (A1, on), (A0_, off), oamg = _pair(mi, oc, dictionary, M)
    assert on.level_value_storage(0, 0)[0] == 8 and off.level_value_storage(0, 0)[0] == 0
    for points in (1, -1):
        assert on.gs_sweep_paths(0, points, True) is not None or mode == 3
    want = None
    if mode == 1:
        want = "gs_tile_k<true, 256>"
    else:
        nr, nc, nnz = mi.c_int(), mi.c_int(), mi.c_big()
        mi.call("HYPRE_MI_BoomerAMGGetLevelCSRSize", on.h, 0, 6, mi.C.byref(nr), mi.C.byref(nc), mi.C.byref(nnz))
        qualifies = nnz.value >= dc.THRESHOLD and nnz.value >= 3 * nr.value
        print(f"{name}: zero-guess sub-operator {nr.value} rows, {nnz.value} entries, kind {on.level_value_storage(0, 6)[0]}")
        assert nr.value == M.shape[0] and on.level_value_storage(0, 6)[0] == (8 if qualifies else 0)
        assert off.level_value_storage(0, 6)[0] == 0
        assert qualifies == (kind == "ragged")
        if qualifies:
            want = "gs_tile_k<true, 256>"
            assert on.gs_sweep_paths(0, 1, True) is not None and on.gs_sweep_paths(0, -1, True) is not None
    _check_zero_pair(mi, kernel_names, on, off, oamg, 950 + len(name) + mode, want)


# ---------------------------------------------------------------- dictionary with fp32 value storage
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", list(dc.PENDANT))
def test_dictionary_with_fp32_value_storage(mi, oc, dictionary, kernel_names, name, mode):
    """Value storage on a level that has a dictionary and whose values are no floats.  The library never narrows level 0
    (HYPRE_MI_BoomerAMGSetValueStorage refuses a first level below 1), so the operator is built for its first coarse
    level to be known: dict_cases.pendant_operator, level 1 = A1 bit for bit.  With the dictionary on, level 1 keeps it
    in every mode (kind 8) and the table is rounded with the values; without it the level streams floats (mode 1) or
    rounded doubles (mode 2).  The doubles multiplied are the same, so relaxation (types 3 and 6: the diagonal they
    divide by is a small integer and does not move) and the level's residual SpMV -- alpha = -1, beta = 1, as relax
    type 11 launches it before its two triangular steps -- agree bit for bit, and with the oracle on the matrix whose
    values went through float."""
    M, A1 = dc.pendant_operator(name)
    w = _width(A1)
    R1 = dc.rounded(A1) if mode else A1
    assert (mode == 0) or not same(R1.data, A1.data)
    (Aon, on), (Aoff, off), oamg = _pair(mi, oc, dictionary, M, mi_value_storage=mode)
    assert on.num_levels > 2
    assert same(np.sort(_level0(on).data), np.sort(M.data)) and off.level_value_storage(0, 0)[0] == 0  # never narrowed
    assert on.level_value_storage(1, 0)[0] == 8 and off.level_value_storage(1, 0)[0] == mode
    # level 1 as the library holds it, back in the order of its rows before the C-first step: R1 exactly
    o1 = oc.Amg(oc.Csr.from_scipy(R1), oc.default_params(gs_chunk=_chunk(mi)))
    import scipy.sparse as sp

    for amg in (on, off):
        ia, ja, a, shape = amg.level_csr(1, 0)
        perm = np.asarray(amg.level_perm(1))
        inv = np.empty_like(perm)
        inv[perm] = np.arange(len(perm))
        U = sp.csr_matrix((a, ja, ia), shape=shape)[inv][:, inv].tocsr()
        U.sort_indices()
        assert np.array_equal(U.indptr, R1.indptr) and np.array_equal(U.indices, R1.indices) and same(U.data, R1.data)
        assert np.array_equal(amg.level_cf(1), o1.level_cf(0)) and np.array_equal(perm, o1.level_perm(0))
        assert amg.gs_sweep_paths(1, 0) is not None
    off_name = "gs_tile_k<false, %d, true>" % w if mode == 1 else None
    _check_relax(mi, kernel_names, on, off, o1, [3, 6], 970 + mode, w, off_name=off_name, level=1)
    _check_relax(mi, kernel_names, on, off, o1, [11], 980 + mode, w, points_list=(0,), off_name=off_name, level=1)
