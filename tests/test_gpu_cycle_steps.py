"""GPU: every step BoomerAMG::cycle runs between two relaxation calls, observed where the cycle runs it
(BoomerAMG.trace_cycle) and held against tests/cycle_steps_ref.py.

Per traced cycle, on every level it reaches:
  * residual, restriction (R through its row map or not), prolongation and the collapsed map applied: per row against the
    long-double reference inside the a-priori bound of a sum of rounded products (nothing measured);
  * the sweeps: bit for bit against relax_pair_level / relax_level on the traced inputs, sweep by sweep;
  * the coarsest dense solve: against the oracle's relax(last, 9) on the library's own levels, at the bar of
    tests/test_gpu_amg.py::test_relax_matches_oracle;
  * the hand-overs between levels (the coarse right-hand side of a second W-cycle visit, the correction, the guess of a
    second visit): bit for bit;
  * what ran (composite or plain residual, skipped zero-fill, dense or swept coarsest level, collapsed or not): read
    from the records' flags and asserted per case.

Grid sizes, chosen on the CPU through the host-only setup (levels as (rows, C rows)): lap7(16) has (4096, 1364), (1364,
328), (328, 102), (102, 25), (25, 5): C counts with nc % 8 == 0 (level 1) and != 0; lap7(13) ends in (13, 2), where
t_from = 8 >= n - 8."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import cycle_steps_ref as ref
from tests import dict_cases as dc
from tests import handover_cases as hc
from tests import systems_cases as sc
from tests.systems import convection_diffusion_3d

pytestmark = pytest.mark.gpu

RATIOS = {"residual": 0.0, "restriction": 0.0, "prolongation": 0.0, "collapsed": 0.0}  # largest error / bound seen


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def first_difference(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64).ravel(), np.ascontiguousarray(b, dtype=np.float64).ravel()
    d = np.flatnonzero(a.view(np.int64) != b.view(np.int64))
    return None if len(d) == 0 else (int(d[0]), float(a[d[0]]), float(b[d[0]]), len(d))


# ---------------------------------------------------------------- operators
def dirichlet_rows(n=14):
    """the convection-diffusion operator with identity rows of tests/test_gpu_amg.py::test_gmres_amg_with_dirichlet_rows"""
    N = n ** 3
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n))
    Cx = sp.diags([-0.4, 0.4], [-1, 0], shape=(n, n))
    I = sp.identity(n)
    M = (sp.kron(sp.kron(I, I), T + Cx) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(T, I), I)).tolil()
    rng = np.random.default_rng(77)
    for i in np.sort(rng.choice(N, size=N // 9, replace=False)):
        M.rows[i], M.data[i] = [int(i)], [1.0]
    M = M.tocsr()
    M.sort_indices()
    return M


def random_mmatrix(n=3000):
    """the seeded random M-matrix of tests/test_gpu_setup_kernels.py::test_device_setup_random_mmatrix"""
    from tests.test_gpu_setup_kernels import _rand_csr

    rng = np.random.default_rng(21)
    B = _rand_csr(rng, n, n, 14)
    B = (B + B.T).tocsr()
    B.data = -np.abs(B.data)
    B.setdiag(0)
    B.eliminate_zeros()
    d = -np.asarray(B.sum(axis=1)).ravel() * (1.0 + 0.05 * rng.random(n)) + 1e-3
    M = (B + sp.diags(d)).tocsr()
    M.sort_indices()
    return M


class Hierarchy:
    """a set-up BoomerAMG with its level operators (fetched once) and the cycle's settings"""

    def __init__(self, mi, oc, M, **kw):
        self.mi, self.oc = mi, oc
        self.A = mi.matrix_from_scipy(sp.csr_matrix(M))
        self.amg = mi.BoomerAMG(print_level=0, **kw)
        self.amg.setup(self.A)
        cfg = self.amg.cfg
        self.types = (cfg.get("down_relax_type", cfg["relax_type"]), cfg.get("up_relax_type", cfg["relax_type"]),
                      cfg.get("coarse_relax_type", 9))
        self.sweeps = (cfg.get("num_down_sweeps", cfg["num_sweeps"]), cfg.get("num_up_sweeps", cfg["num_sweeps"]),
                       cfg.get("num_coarse_sweeps", 1))  # SetNumSweeps leaves the coarsest level at one
        self.relax_order = cfg["relax_order"]
        self.cycle_type = cfg["cycle_type"]
        self.nlev = self.amg.num_levels
        self.ops = [tuple(ref.Csr(*self.amg.level_csr(l, w)) for w in ((0, 2, 3) if l + 1 < self.nlev else (0,)))
                    for l in range(self.nlev)]
        self.n = [o[0].shape[0] for o in self.ops]
        self.info = [self.amg.level_cycle_info(l) for l in range(self.nlev)]
        self._oamg = None
        self.coarsest_A = self.ops[-1][0]  # the operator the dense inverse was taken of

    def oracle(self):
        """the oracle's solve phase on the library's own levels (the coarsest dense solve)"""
        if self._oamg is None:
            oc, mi = self.oc, self.mi
            csr = lambda o: sp.csr_matrix((o.a, o.ja, o.ia), shape=o.shape)
            As = [oc.Csr.from_scipy(csr(self.ops[l][0])) for l in range(self.nlev - 1)] + [oc.Csr.from_scipy(csr(self.coarsest_A))]
            Ps = [oc.Csr.from_scipy(csr(self.ops[l][1])) for l in range(self.nlev - 1)]
            chunk = mi.c_int()
            mi.call("HYPRE_MI_GetGSChunk", mi.C.byref(chunk))
            self._oamg = oc.Amg.from_levels(As, Ps, [self.amg.level_cf(l) for l in range(self.nlev - 1)],
                                            oc.default_params(gs_chunk=chunk.value))
        return self._oamg

    def collapsed_level(self):
        return self.amg.level_cycle_info(0)["collapsed_level"]


class Walk:
    """reads the records of one traced cycle in the order the cycle wrote them and checks every step"""

    def __init__(self, h, recs, label):
        self.h, self.recs, self.pos, self.label = h, recs, 0, label
        self.composite, self.plain, self.fill_skipped, self.collapsed_at = set(), set(), set(), set()
        self.coarsest = None
        self.second_visits = 0

    def take(self, level, step):
        assert self.pos < len(self.recs), (self.label, "the trace ended before", level, step)
        r = self.recs[self.pos]
        assert (r[0], r[2]) == (level, step), (self.label, "record %d is" % self.pos, r[0], r[1], r[2], "expected", level, step)
        assert np.isfinite(r[3]).all(), (self.label, "record %d" % self.pos, r[:3], "is not finite")
        self.pos += 1
        return r

    def peek(self):
        return (self.recs[self.pos][0], self.recs[self.pos][2]) if self.pos < len(self.recs) else None

    def ratio(self, name, v, level):
        assert v, (self.label, name, "level %d" % level, v)
        RATIOS[name] = max(RATIOS[name], v.ratio)

    def replay_sweeps(self, level, which, f, u, zero):
        """the sweeps of a leg through the relaxation hooks, sweep by sweep against the u_sweep records; returns u"""
        h, amg = self.h, self.h.amg
        rtype = h.types[which]
        for sw in range(h.sweeps[which]):
            z = zero and sw == 0
            if which == 2 or h.relax_order != 1:
                got = amg.relax_level(level, rtype, 0, f, np.zeros_like(f) if z else u)
            else:
                got = amg.relax_pair_level(level, rtype, 1 if which == 0 else -1, f, None if z else u)
            r = self.take(level, "u_sweep")
            assert (r[4] >> 8) & 3 == which and r[4] >> 10 == sw and bool(r[4] & amg.TRACE_SWEEP_ZERO) == z, (self.label, r[:3], r[4])
            assert same(r[3], got), (self.label, "sweep %d of leg %d on level %d" % (sw, which, level), first_difference(r[3], got))
            u = r[3]
        return u

    def visit(self, level):
        """one visit of a level; returns (f, u on leaving, zero-guess visit, u on entry)"""
        h, amg = self.h, self.h.amg
        r = self.take(level, "f_in")
        f, flags = r[3], r[4]
        zero = bool(flags & amg.TRACE_ZERO_GUESS)
        if flags & amg.TRACE_FILL_SKIPPED:
            assert zero
            self.fill_skipped.add(level)
        if flags & amg.TRACE_COLLAPSED:
            assert zero
            u = self.take(level, "u_collapsed")[3]
            lt, B = amg.collapsed_tail()
            assert lt == level and B.shape == (h.n[level],) * 2 and h.n[level] <= 1024
            self.ratio("collapsed", ref.check_collapsed(B, f, u), level)
            self.collapsed_at.add(level)
            return f, u, zero, None
        u = np.zeros_like(f) if zero else self.take(level, "u_in")[3]
        u_in = u
        if level == h.nlev - 1:
            before = self.pos
            if h.types[2] == 9 and h.n[level] > 0:
                got = self.take(level, "u_sweep")[3]
                for _ in range(h.sweeps[2] - 1):
                    assert same(self.take(level, "u_sweep")[3], got)  # the same solve of the same f
                r = self.take(level, "u_coarse")
                assert r[4] == amg.TRACE_DENSE and same(r[3], got), (self.label, r[4])
                want = h.oracle().relax(level, 9, 0, f, np.zeros_like(f))
                assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (self.label, "dense solve")
                self.coarsest = "dense"
            else:
                got = self.replay_sweeps(level, 2, f, u, zero)
                r = self.take(level, "u_coarse")
                assert r[4] == amg.TRACE_SWEPT and same(r[3], got), (self.label, r[4])
                self.coarsest = "swept"
            assert self.pos > before
            return f, r[3], zero, u_in
        A, P, R = h.ops[level]
        # down sweeps
        u = self.replay_sweeps(level, 0, f, u, zero and h.sweeps[0] > 0)
        r = self.take(level, "u_down")
        assert same(r[3], u), (self.label, "u_down", level)
        # residual
        r = self.take(level, "resid")
        res = r[3]
        self.ratio("residual", ref.check_residual(A, f, u, res), level)
        if r[4] & amg.TRACE_COMPOSITE:
            # only the F pass of a zero-guess C-then-F pair hands its product over, and only to the next residual
            assert zero and h.sweeps[0] == 1 and h.relax_order == 1 and h.info[level]["has_Ar"], (self.label, level)
            self.composite.add(level)
        else:
            self.plain.add(level)
        # sub-cycle(s): the first one starts from a zero guess on the restricted residual
        visits = []
        while self.peek() != (level + 1, "u_sub"):
            visits.append(self.visit(level + 1))
        e = self.take(level + 1, "u_sub")[3]
        assert len(visits) >= 1 and visits[0][2], (self.label, "the first visit of level %d" % (level + 1))
        self.ratio("restriction", ref.check_restriction(R, res, visits[0][0]), level)
        for q in range(1, len(visits)):  # W-cycle: the same right-hand side, the guess the visit before left
            assert not visits[q][2] and same(visits[q][0], visits[0][0]), (self.label, "visit %d of level %d" % (q, level + 1))
            assert same(visits[q][3], visits[q - 1][1]), (self.label, "the guess of visit %d of level %d" % (q, level + 1))
            self.second_visits += 1
        assert same(e, visits[-1][1]), (self.label, "the correction of level %d" % (level + 1))
        # prolongation
        v = self.take(level, "u_prolong")[3]
        self.ratio("prolongation", ref.check_prolongation(P, u, e, v), level)
        # up sweeps
        u = self.replay_sweeps(level, 1, f, v, False)
        r = self.take(level, "u_up")
        assert same(r[3], u), (self.label, "u_up", level)
        return f, r[3], zero, u_in


def traced(h, level, f, u0=None, collapse=True, label=""):
    """trace one cycle and check every record; returns the Walk (what ran) and the records"""
    recs = h.amg.trace_cycle(level, f, u0, collapse=collapse)
    w = Walk(h, recs, (label, "level %d" % level, "collapse %s" % collapse))
    fin, uout, zero, uin = w.visit(level)
    assert w.pos == len(recs), (label, "records left over", w.pos, len(recs))
    assert same(fin, f) and zero == (u0 is None) and (zero or uin is None or same(uin, u0))
    return w, recs


def rhs(rng, n):
    f = rng.standard_normal(n)
    f[::17] = 0.0
    return f


def check_all_levels(h, seed, label, collapse_modes=(True, False)):
    """a zero-guess cycle from level 0 with the tail collapsed, and one that descends through every level"""
    rng = np.random.default_rng(seed)
    walks = []
    for collapse in collapse_modes:
        w, _ = traced(h, 0, rhs(rng, h.n[0]), None, collapse, label)
        lt = h.collapsed_level()
        if collapse and lt >= 0:
            assert w.collapsed_at == {lt}, (label, w.collapsed_at, lt)
        else:
            assert not w.collapsed_at and w.coarsest is not None
            assert w.composite | w.plain == set(range(h.nlev - 1)), (label, "not every level was reached")
        walks.append(w)
    return walks


@pytest.fixture
def zero_guess_mode(mi):
    try:
        yield lambda mode: mi.call("HYPRE_MI_SetZeroGuessMode", mode)
    finally:
        mi.call("HYPRE_MI_SetZeroGuessMode", 3)


@pytest.fixture
def dictionary(mi):
    try:
        yield mi.set_value_dictionary
    finally:
        mi.set_value_dictionary(True)


@pytest.fixture
def width(mi):
    before = mi.multivector_batch()
    try:
        yield mi.set_multivector_batch
    finally:
        mi.set_multivector_batch(before)


@pytest.fixture
def gs_chunk(mi):
    before = mi.c_int()
    mi.call("HYPRE_MI_GetGSChunk", mi.C.byref(before))
    try:
        yield lambda ch: mi.call("HYPRE_MI_SetGSChunk", ch)
    finally:
        mi.call("HYPRE_MI_SetGSChunk", before.value)


@pytest.fixture
def report():
    yield
    print("largest error / bound so far:", {k: round(v, 4) for k, v in RATIOS.items()})


# ---------------------------------------------------------------- hierarchies
def test_host_built_plain_r(mi, oc, report):
    h = Hierarchy(mi, oc, hc.lap7(16))
    assert h.nlev >= 4 and not any(i["r_row_mapped"] for i in h.info)
    ws = check_all_levels(h, 1, "lap7(16) host")
    print("composite residual on levels", sorted(ws[1].composite), "nc", [h.info[l]["nc"] for l in sorted(ws[1].composite)])
    assert ws[1].coarsest == "dense"


def test_device_built_row_mapped_r(mi, oc, monkeypatch, report):
    """R stored in the fine level's C-point order, written through its row map (asserted through the getter); the
    composite residual on C counts that are and are not multiples of the chunk"""
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    h = Hierarchy(mi, oc, hc.lap7(16))
    mapped = [l for l in range(h.nlev - 1) if h.info[l]["r_row_mapped"]]
    assert 0 in mapped and len(mapped) >= 2, h.info
    assert [(h.n[l], h.info[l]["nc"]) for l in range(2)] == [(4096, 1364), (1364, 328)]
    ws = check_all_levels(h, 2, "lap7(16) device")
    comp = ws[1].composite
    print("row-mapped R on levels", mapped, "composite residual on levels", sorted(comp))
    assert any(h.info[l]["nc"] % 8 == 0 for l in comp) and any(h.info[l]["nc"] % 8 != 0 for l in comp), (comp, h.info)
    for l in comp:
        assert h.info[l]["t_from"] == (h.info[l]["nc"] + 7) // 8 * 8
    assert ws[1].fill_skipped, "no zero-fill was skipped"


def test_composite_residual_where_t_from_reaches_the_end(mi, oc, monkeypatch, report):
    """lap7(13): its last smoothed level has 13 rows and 2 C rows, t_from = 8 >= n - 8"""
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    h = Hierarchy(mi, oc, hc.lap7(13))
    ws = check_all_levels(h, 3, "lap7(13)")
    tails = [l for l in ws[1].composite if h.info[l]["t_from"] >= h.n[l] - 8]
    print("levels (n, nc, t_from):", [(h.n[l], h.info[l]["nc"], h.info[l]["t_from"]) for l in range(h.nlev - 1)],
          "composite", sorted(ws[1].composite))
    assert tails, ("the composite residual never ran where t_from >= n - 8", sorted(ws[1].composite), h.info)


def test_lap27(mi, oc, monkeypatch, report):
    """lap27(12) built on the device.  Its levels have 23, 37 and 28 entries per row (no 27-point Laplacian up to 20^3
    reaches 100 under the suite's coarsenings): the wide tiles are the next test's"""
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    h = Hierarchy(mi, oc, hc.lap27(12))
    assert h.nlev >= 3
    check_all_levels(h, 4, "lap27(12)")


def test_wide_tiles_residual(mi, oc, monkeypatch, report):
    """a smoothed coarse level with >= 100 entries per row (469 rows, 141 per row), so that the 4096-entry tiles run the
    residual: the first coarse level of dict_cases.pendant_operator("wide"), known in advance"""
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    M, A1 = dc.pendant_operator("wide")
    h = Hierarchy(mi, oc, M)
    assert h.nlev >= 3 and h.n[1] == A1.shape[0] and len(h.ops[1][0].a) >= 100 * h.n[1], [len(o[0].a) / o[0].shape[0] for o in h.ops]
    ws = check_all_levels(h, 4, "pendant wide")
    assert 1 in ws[1].composite | ws[1].plain


def test_aggressive_long_rows_of_r(mi, oc, monkeypatch, report):
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    h = Hierarchy(mi, oc, hc.lap7(18), agg_num_levels=1)
    print("longest row of R on level 0:", int(h.ops[0][2].m.max()))
    assert h.ops[0][2].m.max() > h.ops[1][2].m.max() or h.ops[0][2].m.max() >= 16
    check_all_levels(h, 5, "lap7(18) agg")


def test_random_mmatrix(mi, oc, monkeypatch, report):
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    h = Hierarchy(mi, oc, random_mmatrix(), strong_threshold=0.25)
    assert h.nlev > 2
    check_all_levels(h, 6, "random M-matrix")


def test_identity_rows(mi, oc, monkeypatch, report):
    """rows of P without entries (they keep the bits of u) and columns R never reads"""
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    h = Hierarchy(mi, oc, dirichlet_rows(14))
    P, R = h.ops[0][1], h.ops[0][2]
    assert (P.m == 0).sum() >= 14 ** 3 // 9 - 1 and len(np.setdiff1d(np.arange(R.shape[1]), R.ja)) > 0
    check_all_levels(h, 7, "dirichlet rows")


def test_mixed_sign_scaled_operator(mi, oc, monkeypatch, report):
    """aniso16_8_scaled_nonsym: the hand-over case with flagged C rows (C rows with another C column)"""
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    name = "aniso16_8_scaled_nonsym"
    assert hc.CASES[name][3] > 0 and hc.CASES[name][4]
    h = Hierarchy(mi, oc, hc.case(name))
    check_all_levels(h, 8, name)


def test_systems_amg(mi, oc, monkeypatch, report):
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    M, dof, k, _ = sc.case("lame10")
    h = Hierarchy(mi, oc, M, num_functions=3, strong_threshold=sc.THETA)
    assert h.nlev >= 3
    check_all_levels(h, 9, "lame10")


def test_fp32_value_storage(mi, oc, monkeypatch, report):
    """fp32 A, P and R from level 1 on; the reference takes the stored (rounded) values"""
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    h = Hierarchy(mi, oc, hc.lap7(16), mi_value_storage=1)
    assert [h.amg.level_value_storage(1, w)[0] for w in (0, 2, 3)] == [1, 1, 1]
    for w in range(3):
        a = h.ops[1][w].a
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64))
    # the hierarchy is built in fp64 and rounded as the last step of Setup: the dense inverse is
    # that of the unrounded coarsest operator, which the same Setup without value storage reports
    twin = Hierarchy(mi, oc, hc.lap7(16))
    C64, C32 = twin.ops[-1][0], h.ops[-1][0]
    assert twin.nlev == h.nlev and np.array_equal(C64.ia, C32.ia) and np.array_equal(C64.ja, C32.ja)
    assert np.array_equal(C64.a.astype(np.float32).astype(np.float64), C32.a) and not np.array_equal(C64.a, C32.a)
    h.coarsest_A = C64
    check_all_levels(h, 10, "lap7(16) fp32")


def test_air_restriction(mi, oc, monkeypatch, report):
    """restriction=1, interp_type=100: R is not the transpose of P"""
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    h = Hierarchy(mi, oc, convection_diffusion_3d(12), restriction=1, interp_type=100)
    assert h.amg.restriction_info(0)["kind"] in (1, 2)
    P, R = h.ops[0][1], h.ops[0][2]
    Pt = sp.csr_matrix((P.a, P.ja, P.ia), shape=P.shape).T.tocsr()
    Rm = sp.csr_matrix((R.a, R.ja, R.ia), shape=R.shape)
    assert Pt.shape == Rm.shape and abs(Pt - Rm).max() > 0
    check_all_levels(h, 11, "AIR")


@pytest.mark.parametrize("n", [16, 22])
def test_value_dictionary_on_and_off(mi, oc, monkeypatch, dictionary, report, n):
    """lap7(16) with the switch on and off; lap7(22) is the smallest Laplacian whose level 0 has the 65 536 entries from
    which an operator gets a dictionary, so that is where the switch changes the kernels"""
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    kinds = {}
    for on in (True, False):
        dictionary(on)
        h = Hierarchy(mi, oc, hc.lap7(n))
        dictionary(True)
        kinds[on] = h.amg.level_value_storage(0, 0)[0]
        check_all_levels(h, 12, "lap7(%d) dictionary %s" % (n, on))
    assert kinds[False] == 0 and kinds[True] == (8 if n == 22 else 0), kinds


# ---------------------------------------------------------------- settings
def _device_lap16(mi, oc, monkeypatch, **kw):
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    return Hierarchy(mi, oc, hc.lap7(16), **kw)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_zero_guess_modes(mi, oc, monkeypatch, zero_guess_mode, report, mode):
    zero_guess_mode(mode)
    h = _device_lap16(mi, oc, monkeypatch)
    assert all(i["has_Az"] == (mode >= 2) and i["has_Ar"] == (mode == 3) for i in h.info[:-1]), h.info
    ws = check_all_levels(h, 20 + mode, "zero-guess mode %d" % mode)
    w = ws[1]
    print("mode", mode, "composite", sorted(w.composite), "zero-fill skipped", sorted(w.fill_skipped))
    assert bool(w.composite) == (mode == 3)
    if mode == 0:  # only the dense coarsest solve ignores its u
        assert w.fill_skipped <= {h.nlev - 1}


def test_non_zero_guess(mi, oc, monkeypatch, report):
    h = _device_lap16(mi, oc, monkeypatch)
    rng = np.random.default_rng(30)
    for level in (0, 1):
        for collapse in (True, False):
            w, recs = traced(h, level, rhs(rng, h.n[level]), rng.standard_normal(h.n[level]), collapse, "u0")
            assert level in w.plain and level not in w.composite  # a non-zero guess: the plain residual
            assert recs[1][2] == "u_in"
    # the collapsed level itself with a guess: it must cycle, not apply the map
    lt = h.collapsed_level()
    assert lt >= 1
    w, _ = traced(h, lt, rhs(rng, h.n[lt]), rng.standard_normal(h.n[lt]), True, "u0 on the collapsed level")
    assert not w.collapsed_at and lt in w.plain


def test_w_cycle_second_visit_takes_the_plain_residual(mi, oc, monkeypatch, report):
    h = _device_lap16(mi, oc, monkeypatch, cycle_type=2)
    rng = np.random.default_rng(31)
    recs = h.amg.trace_cycle(0, rhs(rng, h.n[0]), collapse=False)
    w = Walk(h, recs, "W-cycle")
    w.visit(0)
    assert w.pos == len(recs) and w.second_visits >= 2
    amg = h.amg
    zero_of = {}
    seen_second = 0
    for r in recs:
        if r[2] == "f_in":
            zero_of[(r[0], r[1])] = bool(r[4] & amg.TRACE_ZERO_GUESS)
        if r[2] == "resid":
            comp = bool(r[4] & amg.TRACE_COMPOSITE)
            if not zero_of[(r[0], r[1])]:
                seen_second += 1
                assert not comp, ("a visit with a non-zero guess ran the composite residual", r[0], r[1])
    assert seen_second >= 1 and w.composite
    # every zero-guess visit of a level that runs the composite residual runs it, every other visit does not
    for l in w.composite:
        flags = [(zero_of[(r[0], r[1])], bool(r[4] & amg.TRACE_COMPOSITE)) for r in recs if r[2] == "resid" and r[0] == l]
        assert all(z == c for z, c in flags), (l, flags)
    traced(h, 0, rhs(rng, h.n[0]), None, True, "W-cycle collapsed")


def test_two_sweeps_invalidate_the_handed_over_product(mi, oc, monkeypatch, report):
    h = _device_lap16(mi, oc, monkeypatch, num_down_sweeps=2, num_up_sweeps=2, num_coarse_sweeps=1)
    ws = check_all_levels(h, 32, "two sweeps")
    assert not ws[0].composite and not ws[1].composite


def test_relax_order_0(mi, oc, monkeypatch, report):
    h = _device_lap16(mi, oc, monkeypatch, relax_order=0)
    ws = check_all_levels(h, 33, "relax_order 0")
    assert not ws[1].composite


def test_l1_jacobi_has_no_sub_operators(mi, oc, monkeypatch, report):
    h = _device_lap16(mi, oc, monkeypatch, relax_type=18)
    assert not any(i["has_Az"] or i["has_Ar"] for i in h.info)
    ws = check_all_levels(h, 34, "relax_type 18")
    assert not ws[1].composite and ws[1].fill_skipped <= {h.nlev - 1}


@pytest.mark.parametrize("max_coarse", [9, 200])
def test_max_coarse_size(mi, oc, monkeypatch, report, max_coarse):
    h = _device_lap16(mi, oc, monkeypatch, max_coarse_size=max_coarse)
    assert h.n[-1] <= max_coarse < h.n[-2]
    ws = check_all_levels(h, 35, "max_coarse_size %d" % max_coarse)
    assert ws[1].coarsest == "dense"


def test_swept_coarsest_level(mi, oc, monkeypatch, report):
    h = _device_lap16(mi, oc, monkeypatch, down_relax_type=8, up_relax_type=8, coarse_relax_type=8)
    ws = check_all_levels(h, 36, "coarse_relax_type 8")
    assert ws[1].coarsest == "swept"


def test_gs_chunk_4_takes_the_plain_residual(mi, oc, monkeypatch, gs_chunk, report):
    """the sub-operators were cut for chunks of 8: with another chunk nothing is handed over"""
    h = _device_lap16(mi, oc, monkeypatch)
    gs_chunk(4)
    h._oamg = None
    ws = check_all_levels(h, 37, "gs chunk 4")
    assert not ws[0].composite and not ws[1].composite
    gs_chunk(8)
    ws = check_all_levels(h, 37, "gs chunk back at 8")
    assert ws[1].composite


# ---------------------------------------------------------------- bit-for-bit comparisons
def test_collapsed_map_columns_are_the_traced_unit_cycles(mi, oc, monkeypatch, report):
    """column j of the tabulated map = the u of cycle(lt, e_j) through the level: j = 0 is the plain launch, 1 and 2 the
    first graph replays, n - 1 the last, eight seeded others"""
    h = _device_lap16(mi, oc, monkeypatch)
    lt, B = h.amg.collapsed_tail()
    n = h.n[lt]
    assert lt >= 1 and B.shape == (n, n) and n <= 1024
    rng = np.random.default_rng(40)
    cols = [0, 1, 2, n - 1] + sorted(int(j) for j in rng.choice(np.arange(3, n - 1), size=8, replace=False))
    for j in cols:
        e = np.zeros(n)
        e[j] = 1.0
        recs = h.amg.trace_cycle(lt, e, collapse=False)
        assert recs[-1][0] == lt and recs[-1][2] == "u_up"
        assert same(recs[-1][3], B[:, j]), ("column %d of the collapsed map" % j, first_difference(recs[-1][3], B[:, j]))


def test_batched_trace_equals_the_single_vector_traces(mi, oc, monkeypatch, width, report):
    from tests.test_gpu_multivector_batch import _vectors

    h = _device_lap16(mi, oc, monkeypatch)
    width(4)
    rng = np.random.default_rng(41)
    for level, collapse, guess in ((0, True, False), (0, False, False), (0, False, True), (1, False, False)):
        F = _vectors(rng, 3, h.n[level])
        U = _vectors(rng, 3, h.n[level])[::-1].copy() if guess else None
        multi = h.amg.trace_cycle(level, F, U, nvec=3, collapse=collapse)
        for c in range(3):
            one = h.amg.trace_cycle(level, F[c], None if U is None else U[c], collapse=collapse)
            assert [r[:3] + (r[4],) for r in one] == [r[:3] + (r[4],) for r in multi], (level, collapse, guess, c)
            for i, (a, b) in enumerate(zip(one, multi)):
                assert same(a[3], b[3][c]), (level, collapse, guess, "component %d, record %d" % (c, i), a[:3],
                                            first_difference(a[3], b[3][c]))
        if U is None:  # the all-zero component stayed zero beside the huge one
            assert not multi[-1][3][2].any() and np.abs(multi[-1][3][0]).max() > 1e140


def test_poisoned_work_vectors(mi, oc, monkeypatch, report):
    h = _device_lap16(mi, oc, monkeypatch)
    rng = np.random.default_rng(42)
    f = rhs(rng, h.n[0])
    for collapse in (True, False):
        clean = h.amg.trace_cycle(0, f, collapse=collapse)
        mi.call("HYPRE_MI_BoomerAMGPoisonWorkVectors", h.amg.h)
        dirty = h.amg.trace_cycle(0, f, collapse=collapse)
        assert any(r[4] & h.amg.TRACE_FILL_SKIPPED for r in clean if r[2] == "f_in")
        assert [r[:3] + (r[4],) for r in clean] == [r[:3] + (r[4],) for r in dirty]
        for i, (a, b) in enumerate(zip(clean, dirty)):
            assert np.isfinite(b[3]).all() and same(a[3], b[3]), (collapse, "record %d" % i, a[:3], first_difference(a[3], b[3]))


def test_trace_refusals(mi, oc):
    h = Hierarchy(mi, oc, hc.lap7(9))
    for args in ((h.nlev, np.zeros(4)), (-1, np.zeros(4))):
        with pytest.raises(mi.HypreError, match="level"):
            h.amg.trace_cycle(*args)
        mi.call("HYPRE_ClearAllErrors")
    with pytest.raises(mi.HypreError, match="nvec"):
        h.amg.trace_cycle(0, np.zeros((5, h.n[0])), nvec=5)
    mi.call("HYPRE_ClearAllErrors")
