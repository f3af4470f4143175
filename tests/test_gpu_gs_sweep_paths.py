"""The tile Gauss-Seidel kernel leaves the in-chunk sweep out where it would only multiply structural zeros:
waves without a selected row, waves whose chunks couple to nothing in-chunk but their diagonals, and (forward) tiles
that start from a zero guess.  Each case against the oracle's relaxation, 1e-12 relative to max|u| as
test_relax_matches_oracle in test_gpu_amg.py has it.

The operators are built so that the case in question is certainly met: `_stride_operator` couples row i only to rows
i +- 64 m, which stay at least 8 rows away in the level's C-first ordering, so every 8-row chunk of level 0 is
diagonal; one planted weak coupling puts exactly one chunk (one wave) back on the general sweep.  Every test checks
that structure on the level operator it got back from the library, and reads the branch each wave takes from the
host-side census (HYPRE_MI_BoomerAMGGetGSSweepPaths), which evaluates the kernel's predicates on the same launch
geometry.  In one-tile cases the census itself is checked against a count made here.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RELAX_TYPES = [3, 4, 6, 8, 13, 14]
TOL = 1e-12


def _chunk(mi):
    c = mi.c_int()
    mi.call("HYPRE_MI_GetGSChunk", mi.C.byref(c))
    return c.value


def _stride_operator(n, nstrides, planted=()):
    """Symmetric M-matrix: row i couples to i +- 64 m, m = 1..nstrides, with weights in [0.75, 1.25] (all strong at
    the default threshold), weakly dominant diagonal.  planted: extra pairs (i, j) with a WEAK coupling (1e-3: below
    the strength threshold, so the C/F splitting does not move)."""
    import scipy.sparse as sp

    i = np.arange(n)
    rows, cols, vals = [], [], []
    for m in range(1, nstrides + 1):
        lo = i[: n - 64 * m]
        hi = lo + 64 * m
        w = -(1.0 + 0.25 * np.sin(0.37 * lo + 1.3 * m))
        rows += [lo, hi]
        cols += [hi, lo]
        vals += [w, w]
    for (p, q) in planted:
        rows += [np.array([p, q])]
        cols += [np.array([q, p])]
        vals += [np.array([-1e-3, -1e-3])]
    M = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    M = (M + sp.diags(np.abs(M).sum(axis=1).A1 * 1.02 + 0.05)).tocsr()
    M.sort_indices()
    return M


@pytest.fixture
def zero_mode_1(mi):
    """Zero-guess sweeps on the level operator itself (zero_from tells the kernel where the zeros start) rather than on
    the zero-guess sub-operator, whose short rows may take it off the tile kernel; for hierarchies set up inside."""
    mi.call("HYPRE_MI_SetZeroGuessMode", 1)
    yield
    mi.call("HYPRE_MI_SetZeroGuessMode", 3)


def _setup(mi, oc, M, **kw):
    n = M.shape[0]
    A = mi.IJMatrix(0, n - 1)
    coo = M.tocoo()
    A.set_values_coo(coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data)
    A.assemble()
    amg = mi.BoomerAMG(print_level=0, **kw)
    amg.setup(A)
    oamg = oc.Amg(oc.Csr.from_scipy(M), oc.default_params(gs_chunk=_chunk(mi), **kw))
    assert amg.num_levels == oamg.num_levels and amg.num_levels > 1
    assert np.array_equal(amg.level_cf(0), oamg.level_cf(0))
    assert np.array_equal(amg.level_perm(0), oamg.level_perm(0))
    return A, amg, oamg


def _level_pattern(amg, level=0):
    """(rows, cols) of the level operator's entries in the level's own (C-first) ordering, and nc."""
    ia, ja, a, shape = amg.level_csr(level, 0)
    rows = np.repeat(np.arange(shape[0]), np.diff(ia))
    nc = int((np.asarray(amg.level_cf(level)) == 1).sum())
    return rows, np.asarray(ja), nc


def _coupled_chunks(amg, level=0):
    """chunks (row // 8) of the level that hold an in-chunk entry off the diagonal"""
    rows, ja, nc = _level_pattern(amg, level)
    off = (rows // 8 == ja // 8) & (rows != ja)
    return np.unique(rows[off] // 8)


def _check_relax(mi, amg, oamg, level, rtypes, seed, points_list=(0, 1, -1)):
    n = oamg.level_A(level).shape[0]
    rng = np.random.default_rng(seed)
    cf = oamg.level_cf(level)
    for rtype in rtypes:
        f, u0 = rng.standard_normal(n), rng.standard_normal(n)
        for points in points_list:
            got = amg.relax_level(level, rtype, points, f, u0)
            ref = oamg.relax(level, rtype, points, f, u0)
            err = np.abs(got - ref).max()
            print(f"level {level} type {rtype} points {points}: max err {err:.3e} (max|ref| {np.abs(ref).max():.3e})")
            assert err <= TOL * max(1.0, np.abs(ref).max())
            if points != 0:
                assert np.array_equal(got[cf != points], u0[cf != points])


def _check_zero_pair(amg, oamg, level, rtypes, seed):
    """first sweep of a down leg: C pass then F pass from u = 0"""
    n = oamg.level_A(level).shape[0]
    rng = np.random.default_rng(seed)
    for rtype in rtypes:
        f = rng.standard_normal(n)
        got = amg.relax_pair_level(level, rtype, 1, f)
        ref = oamg.relax(level, rtype, -1, f, oamg.relax(level, rtype, 1, f, np.zeros(n)))
        err = np.abs(got - ref).max()
        print(f"level {level} type {rtype} zero-guess C-then-F: max err {err:.3e} (max|ref| {np.abs(ref).max():.3e})")
        assert err <= TOL * max(1.0, np.abs(ref).max())
        # ... and the same pair from a given vector (no zero-guess path), both orders
        u0 = rng.standard_normal(n)
        for first in (1, -1):
            got = amg.relax_pair_level(level, rtype, first, f, u0)
            ref = oamg.relax(level, rtype, -first, f, oamg.relax(level, rtype, first, f, u0))
            assert np.abs(got - ref).max() <= TOL * max(1.0, np.abs(ref).max())


# (strides, rows): entries per row 2 * strides + 1 -> rows per 2048-entry tile -> lanes per row (LPR) and idle waves
GEOMETRIES = [
    pytest.param(3, 4096, 1, False, id="rowlen7-LPR1"),
    pytest.param(8, 4096, 2, False, id="rowlen17-LPR2"),
    pytest.param(16, 4096, 4, False, id="rowlen33-LPR4"),
    pytest.param(32, 8192, 8, True, id="rowlen65-LPR8-24rows-1idle"),
    pytest.param(46, 8100, 8, True, id="rowlen93-LPR8-16rows-2idle"),
]


@pytest.mark.parametrize("nstrides,n,lpr,idle", GEOMETRIES)
def test_diagonal_chunks_every_geometry(mi, oc, zero_mode_1, nstrides, n, lpr, idle):
    """Every chunk of level 0 is diagonal: no wave runs the 16-step sweep, in any pass, whatever LPR the tiles have;
    tiles of 24 / 16 rows leave one / two of their four waves without rows."""
    M = _stride_operator(n, nstrides)
    A, amg, oamg = _setup(mi, oc, M)
    assert len(_coupled_chunks(amg)) == 0
    rows, ja, nc = _level_pattern(amg)
    assert 0 < nc < n and nc % 8 != 0
    for points in (0, 1, -1):
        for zero in (False, True):
            c = amg.gs_sweep_paths(0, points, zero)
            print(f"strides {nstrides} points {points} zero {zero}: {c}")
            assert c is not None, "the pass must run on the tile kernel"
            assert c["general"] == 0 and c["zero"] == 0 and c["diagonal"] > 0
            assert c["idle"] + c["diagonal"] == c["waves"]
    c = amg.gs_sweep_paths(0, 0)
    # the rows in the middle of the band have 2 * strides + 1 entries (fewer towards both ends, so the tiles there hold
    # more rows at fewer lanes each): at least n / 64 busy waves, more where LPR > 1, and idle ones in tiles of <= 24 rows
    assert c["diagonal"] >= n // 64
    if lpr > 1:
        assert c["diagonal"] > n // 64 + 8
    if idle:
        assert c["idle"] > 8
    _check_relax(mi, amg, oamg, 0, RELAX_TYPES, 300 + nstrides)
    _check_zero_pair(amg, oamg, 0, RELAX_TYPES, 400 + nstrides)


@pytest.mark.parametrize("nstrides,n", [(3, 4096), (16, 4096), (32, 8192)])
@pytest.mark.parametrize("where", ["F", "C-straddle"])
def test_one_planted_coupling_falls_back(mi, oc, zero_mode_1, nstrides, n, where):
    """One weak in-chunk coupling in ONE chunk: exactly the wave that holds it runs the general sweep (the other
    waves of its tile stay on the diagonal path -- a tile with both kinds), and only in passes that select its rows."""
    A0, amg0, oamg0 = _setup(mi, oc, _stride_operator(n, nstrides))
    perm = np.asarray(amg0.level_perm(0))  # perm[new] = old
    cf0 = np.asarray(amg0.level_cf(0))
    nc = int((cf0 == 1).sum())
    if where == "F":
        p = (nc + 7) // 8 * 8 + 8 * 37 + 2  # two F rows of one chunk, well inside the F block
        q = p + 3
    else:
        assert nc % 8 not in (0, 7)
        p, q = nc - 1, nc  # the last C row and the first F row share the chunk that straddles nc
    assert p // 8 == q // 8
    M = _stride_operator(n, nstrides, planted=[(int(perm[p]), int(perm[q]))])
    A, amg, oamg = _setup(mi, oc, M)
    assert np.array_equal(amg.level_perm(0), perm) and np.array_equal(amg.level_cf(0), cf0)
    assert list(_coupled_chunks(amg)) == [p // 8]
    for points in (0, 1, -1):
        c = amg.gs_sweep_paths(0, points)
        print(f"{where} strides {nstrides} points {points}: {c}")
        selected = points == 0 or (where == "C-straddle") or points == -1
        assert c["general"] == (1 if selected else 0) and c["zero"] == 0
        assert c["idle"] + c["diagonal"] + c["general"] == c["waves"] and c["diagonal"] > 0
    # zero guess: the F block's tiles start at or after nc -> the short forward sweep; the straddling tile starts
    # before nc -> the general one
    cz = amg.gs_sweep_paths(0, -1, True)
    print(f"{where} strides {nstrides} zero-guess F pass: {cz}")
    assert cz["zero"] + cz["general"] == 1
    assert (cz["general"] == 1) == (where == "C-straddle")
    _check_relax(mi, amg, oamg, 0, RELAX_TYPES, 500 + nstrides)
    _check_zero_pair(amg, oamg, 0, RELAX_TYPES, 600 + nstrides)


def test_census_matches_a_direct_count(mi, oc):
    """One tile (200 rows of about 8 entries: LPR 1, rows 0..63 in wave 0, ...): the census against a count made here."""
    n = 200
    import scipy.sparse as sp

    rng = np.random.default_rng(5)
    M = sp.random(n, n, density=0.017, random_state=rng, format="csr")
    M = -abs(M + M.T)
    M.setdiag(0.0)
    M.eliminate_zeros()
    M = (M + sp.diags(np.abs(M).sum(axis=1).A1 * 1.05 + 0.1)).tocsr()
    M.sort_indices()
    A, amg, oamg = _setup(mi, oc, M)
    rows, ja, nc = _level_pattern(amg)
    cf = np.asarray(amg.level_cf(0))
    assert 128 < n <= 256 and len(ja) < 2048 and len(ja) > 5 * n
    coupled_row = np.zeros(n, dtype=bool)
    coupled_row[rows[(rows // 8 == ja // 8) & (rows != ja)]] = True
    for points in (0, 1, -1):
        lo, hi = (nc if points == -1 else 0), (nc if points == 1 else n)
        lo, hi = lo // 8 * 8, min((hi + 7) // 8 * 8, n)
        sel = (np.arange(n) >= lo) & (np.arange(n) < hi) & ((cf == points) | (points == 0))
        want = dict(waves=4, idle=0, diagonal=0, zero=0, general=0)
        for w in range(4):
            r = slice(w * 64, min((w + 1) * 64, n))  # LPR 1 for 129..256 rows
            if not sel[r].any():
                want["idle"] += 1
            elif not (coupled_row[r] & sel[r]).any():
                want["diagonal"] += 1
            else:
                want["general"] += 1
        got = amg.gs_sweep_paths(0, points)
        print(points, got, want)
        assert got == want
    assert amg.gs_sweep_paths(0, 0)["general"] > 0
    _check_relax(mi, amg, oamg, 0, RELAX_TYPES, 700)
    _check_zero_pair(amg, oamg, 0, RELAX_TYPES, 701)


@pytest.mark.parametrize("n,stencil", [(14, 7), (20, 7), (12, 27)])
def test_zero_guess_pairs_on_laplace_levels(mi, oc, n, stencil):
    """Zero-guess C-then-F pairs on the levels of a Laplace hierarchy (coupled chunks: the short forward sweep and,
    in the tile that straddles nc, the general one), all relax types, and the same levels from a given vector."""
    A, b, x, rhs = mi.build_laplace_system(n, n, n, stencil)
    amg = mi.BoomerAMG(print_level=0)
    amg.setup(A)
    Ao, bo = oc.Csr.laplace(n, n, n, stencil)
    oamg = oc.Amg(Ao, oc.default_params(gs_chunk=_chunk(mi)))
    assert amg.num_levels == oamg.num_levels
    seen = dict(zero=0, general=0, diagonal=0, idle=0)
    straddle = False
    for level in range(min(3, amg.num_levels - 1)):
        rows, ja, nc = _level_pattern(amg, level)
        for points in (1, -1):
            c = amg.gs_sweep_paths(level, points, True)
            print(f"n {n} stencil {stencil} level {level} points {points} zero guess: {c} (nc {nc}, nc % 8 = {nc % 8})")
            if c is not None:
                straddle |= points == -1 and nc % 8 != 0
                for k in seen:
                    seen[k] += c[k]
        _check_zero_pair(amg, oamg, level, RELAX_TYPES, 800 + level)
        _check_relax(mi, amg, oamg, level, RELAX_TYPES, 810 + level)
    assert seen["zero"] > 0 and seen["diagonal"] > 0
    assert straddle and seen["general"] > 0  # a tile that straddles nc inside a chunk, on the general sweep


def test_gmres_amg_on_diagonal_chunk_operator_matches_oracle(mi, oc):
    """A whole solve behind the new branches (level 0: diagonal chunks and idle waves in every pass; one planted
    coupling; coarser levels: whatever the hierarchy gives): iteration count and residual history as the oracle's,
    by the rule of test_gmres_amg_matches_oracle (1e-8 relative per step, no absolute floor).

    Solver tolerance 1e-8, as that test's own GMRES(50) cases have it.  The rule has no rounding floor, so it holds
    down to about eight orders of reduction and not below: run to 1e-10 this system (|r0| = 5.3e3) takes 8 steps, steps
    0-7 agree with the oracle to better than 1e-9 and step 8 -- 4.56496425e-08 against 4.56496444e-08, eleven orders
    below |r0| -- differs by 4.2e-8 relative, 1.9e-15 absolute = 3.6e-19 |r0|: the device's and the oracle's different
    summation orders, far below the 1e-14 |r0| floor that test_gmres_amg_other_hierarchies_match_oracle allows."""
    n, nstrides, tol = 8192, 32, 1e-8
    A0, amg0, oamg0 = _setup(mi, oc, _stride_operator(n, nstrides))
    perm = np.asarray(amg0.level_perm(0))
    nc = int((np.asarray(amg0.level_cf(0)) == 1).sum())
    p = (nc + 7) // 8 * 8 + 8 * 11 + 1
    M = _stride_operator(n, nstrides, planted=[(int(perm[p]), int(perm[p + 5]))])
    rng = np.random.default_rng(9)
    xs = rng.standard_normal(n)
    bv = M @ xs
    A = mi.IJMatrix(0, n - 1)
    coo = M.tocoo()
    A.set_values_coo(coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data)
    A.assemble()
    b = mi.IJVector(0, n - 1, bv)
    x = mi.IJVector(0, n - 1, np.zeros(n))
    amg = mi.BoomerAMG(print_level=0)
    gm = mi.GMRES(tolerance=tol, max_iterations=100, kspace=30, print_level=0)
    gm.set_precond(amg)
    gm.setup(A, b, x)
    assert gm.solve(A, b, x) == 0
    c = amg.gs_sweep_paths(0, -1)
    assert c is not None and c["general"] == 1 and c["diagonal"] > 0 and c["idle"] > 0
    Ao = oc.Csr.from_scipy(M)
    oamg = oc.Amg(Ao, oc.default_params(gs_chunk=_chunk(mi)))
    xo, info = oc.gmres(Ao, bv, kdim=30, tol=tol, maxit=100, amg=oamg)
    hist = gm.residual_history()
    print(f"iterations {gm.num_iterations} / oracle {info['iters']}; final rel res {gm.final_rel_res:.3e} / {info['rel_res']:.3e}")
    assert gm.num_iterations == info["iters"] and gm.num_iterations > 2
    assert len(hist) == len(info["norms"])
    assert np.allclose(hist, info["norms"], rtol=1e-8, atol=0.0)
    assert abs(gm.final_rel_res - info["rel_res"]) <= 1e-10
    assert np.abs(x.get() - xo).max() <= 1e-8 * max(1.0, np.abs(xo).max())
    # true residual of the device solution, by the oracle's SpMV
    assert np.linalg.norm(bv - Ao.matvec(x.get())) / np.linalg.norm(bv) <= tol * 1.0000001
