"""CPU: the specification of setup reuse (HYPRE_MI_BoomerAMGSetSetupReuse; DESIGN.md section 3, "Setup reuse") through
HYPRE_MI_IJMatrixAssembleHostOnly, host update rounds and HYPRE_MI_BoomerAMGSetupHostOnly.  A refresh keeps cf, the
permutations, P and R bit for bit and gives every level operator the bits of the restatement in tests/setup_reuse_ref.py
(explicit loops in the contract's order) on the stored pattern; against scipy's product the bound is
1e-13 (|P^T| |A| |P|)_ij: an entry sums at most a few hundred products, each rounded to 2^-53 relative."""
import numpy as np
import pytest

from tests import ij_cases as cases
from tests import ij_update_cases as upd
from tests import setup_reuse_cases as rc
from tests import setup_reuse_ref as ref

SYSTEMS = ["lap7_8", "lap27_6", "convdiff8", "mmatrix400"]
KW = {"mmatrix400": dict(strong_threshold=0.25)}


def host_matrix(mi, M):
    return cases.host_only_matrix(mi, M.shape[0], [rc.triples(M) + (False,)])


def update(mi, A, M):
    upd.apply_round(mi, A, [rc.triples(M) + (False,)], host_only=True)


def host_setup(mi, amg, A):
    mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)


def new_amg(mi, name, reuse=1, **kw):
    cfg = dict(KW.get(name, {}), **kw)
    if reuse is not None:
        cfg["setup_reuse"] = reuse
    return mi.BoomerAMG(print_level=0, **cfg)


def refreshed(mi, name, M0, M1):
    """(snapshot after the first Setup on M0, snapshot after an update round to M1 and a second Setup, handles)"""
    A = host_matrix(mi, M0)
    amg = new_amg(mi, name)
    host_setup(mi, amg, A)
    assert amg.setup_kind() == (1, 1)
    before = rc.snapshot(amg)
    update(mi, A, M1)
    host_setup(mi, amg, A)
    return before, rc.snapshot(amg), amg, A


def check_against_restatement(before, after, M1):
    assert len(before) == len(after) >= 2
    A_prev = None
    for l, (b, a) in enumerate(zip(before, after)):
        assert np.array_equal(b["perm"], a["perm"])
        assert rc.same_csr(b["A"], a["A"], values=False)
        if l == 0:
            perm = a["perm"]
            want = ref.lookup_through_permutation(M1, ref.csr(*a["A"]), perm, perm)
            assert None not in want and np.array_equal(np.array(want).view(np.int64), a["A"][2].view(np.int64))
        else:
            P = ref.csr(*before[l - 1]["P"])
            vals, fits = ref.triple_product_into_pattern(A_prev, P, ref.csr(*a["A"]))
            assert fits and np.array_equal(vals.view(np.int64), a["A"][2].view(np.int64)), l
            C, B = ref.triple_product_scipy(A_prev, P)
            got = ref.csr(*a["A"])
            assert np.array_equal(C.indptr, got.indptr) and np.array_equal(C.indices, got.indices)
            assert (np.abs(C.data - got.data) <= 1e-13 * B.data).all(), l
        A_prev = ref.csr(*a["A"])
        d, l1 = ref.diag_and_l1(A_prev)
        assert rc.same_bits(a["norms"][0], d) and rc.same_bits(a["norms"][2], l1)
        if "P" in b:
            assert rc.same_csr(b["P"], a["P"]) and rc.same_csr(b["R"], a["R"]) and np.array_equal(b["cf"], a["cf"])


@pytest.mark.parametrize("name", SYSTEMS)
@pytest.mark.parametrize("change", ["a", "c", "d"])
def test_refresh_keeps_the_structure_and_has_the_bits_of_the_restatement(mi_lib, oc, name, change):
    mi = mi_lib
    M0 = rc.system(oc, name)
    M1 = rc.changed(M0, change)
    if change == "d":
        assert len(np.unique(M1.data)) > 256
    full0, refreshed0 = mi.counter("amg_setups_full"), mi.counter("amg_setups_refreshed")
    before, after, amg, A = refreshed(mi, name, M0, M1)
    assert amg.setup_kind() == (2, 0)
    assert mi.counter("amg_setups_full") == full0 + 1 and mi.counter("amg_setups_refreshed") == refreshed0 + 1
    check_against_restatement(before, after, M1)


@pytest.mark.parametrize("name", SYSTEMS)
def test_unchanged_values_agree_with_a_fresh_handle_to_rounding(mi_lib, oc, name):
    """the fresh setup multiplies in natural order and renumbers afterwards: other k and m orders, so rounding, not bits;
    GMRES(20) to 1e-9 preconditioned by the oracle's cycle on either hierarchy takes the same number of iterations"""
    mi = mi_lib
    M0 = rc.system(oc, name)
    before, after, amg, A = refreshed(mi, name, M0, M0)
    assert amg.setup_kind() == (2, 0)
    for l in range(1, len(after)):
        P = ref.csr(*before[l - 1]["P"])
        _, B = ref.triple_product_scipy(ref.csr(*after[l - 1]["A"]), P)
        assert rc.same_csr(before[l]["A"], after[l]["A"], values=False)
        assert (np.abs(before[l]["A"][2] - after[l]["A"][2]) <= 1e-13 * B.data).all()
    chunk = mi.c_int()
    mi.call("HYPRE_MI_GetGSChunk", mi.C.byref(chunk))
    iters = []
    for snap in (before, after):
        As = [oc.Csr.from_scipy(ref.csr(*d["A"])) for d in snap]
        Ps = [oc.Csr.from_scipy(ref.csr(*d["P"])) for d in snap[:-1]]
        oamg = oc.Amg.from_levels(As, Ps, [d["cf"] for d in snap[:-1]],
                                  oc.default_params(gs_chunk=chunk.value, **KW.get(name, {})))
        b = np.cos(np.arange(M0.shape[0], dtype=np.float64))
        x, info = oc.gmres(As[0], b, kdim=20, tol=1e-9, maxit=100, amg=oamg)
        iters.append(info["iters"])
    print(name, "GMRES(20) iterations, fresh and refreshed:", iters)
    assert iters[0] == iters[1] and iters[0] < 100


@pytest.mark.parametrize("name", ["lap7_8", "convdiff8"])
def test_no_state_of_an_intermediate_matrix_survives(mi_lib, oc, name):
    mi = mi_lib
    M0 = rc.system(oc, name)
    _, direct, _, _ = refreshed(mi, name, M0, M0)
    A = host_matrix(mi, M0)
    amg = new_amg(mi, name)
    host_setup(mi, amg, A)
    for M in (rc.changed(M0, "d"), M0):
        update(mi, A, M)
        host_setup(mi, amg, A)
        assert amg.setup_kind() == (2, 0)
    there_and_back = rc.snapshot(amg)
    for x, y in zip(direct, there_and_back):
        assert rc.same_csr(x["A"], y["A"]) and all(rc.same_bits(p, q) for p, q in zip(x["norms"], y["norms"]))


@pytest.mark.parametrize("name", SYSTEMS)
def test_powers_of_two_scale_every_operator_and_norm_exactly(mi_lib, oc, name):
    mi = mi_lib
    M0 = rc.system(oc, name)
    _, base, _, _ = refreshed(mi, name, M0, M0)
    for change, s in (("b8", 0.125), ("b2", 2.0)):
        _, got, amg, _ = refreshed(mi, name, M0, rc.changed(M0, change))
        assert amg.setup_kind() == (2, 0)
        for x, y in zip(base, got):
            assert rc.same_bits(x["A"][2] * s, y["A"][2])
            assert all(rc.same_bits(p * s, q) for p, q in zip(x["norms"], y["norms"]))


def test_every_reason_of_a_rebuild_and_the_bad_mode(mi_lib, oc):
    mi = mi_lib
    name = "lap7_8"
    M0 = rc.system(oc, name)
    M1 = rc.changed(M0, "c")

    def never_switched(M, **kw):
        h = new_amg(mi, name, reuse=None, **kw)
        host_setup(mi, h, host_matrix(mi, M))
        assert h.setup_kind() == (1, 0)
        return rc.snapshot(h)

    def same_hierarchy(x, y):
        return len(x) == len(y) and all(
            rc.same_csr(p["A"], q["A"]) and np.array_equal(p["perm"], q["perm"]) and
            all(rc.same_bits(u, v) for u, v in zip(p["norms"], q["norms"])) and
            ("P" not in p or (rc.same_csr(p["P"], q["P"]) and np.array_equal(p["cf"], q["cf"]))) for p, q in zip(x, y))

    plain1 = never_switched(M1)
    # never set up; reason 0: the switch is off, twice on one handle
    amg = new_amg(mi, name, reuse=0)
    assert amg.setup_kind() == (0, 0)
    A = host_matrix(mi, M0)
    host_setup(mi, amg, A)
    update(mi, A, M1)
    host_setup(mi, amg, A)
    assert amg.setup_kind() == (1, 0) and same_hierarchy(rc.snapshot(amg), plain1)
    # reason 1, then reason 2: another matrix object with the same pattern and values
    amg = new_amg(mi, name)
    host_setup(mi, amg, A)
    assert amg.setup_kind() == (1, 1)
    B = host_matrix(mi, M1)
    host_setup(mi, amg, B)
    assert amg.setup_kind() == (1, 2) and same_hierarchy(rc.snapshot(amg), plain1)
    # reason 3: a structural setting changed (and the rebuild is the changed setting's hierarchy)
    mi.call("HYPRE_BoomerAMGSetStrongThreshold", amg.h, 0.9)
    host_setup(mi, amg, B)
    assert amg.setup_kind() == (1, 3) and same_hierarchy(rc.snapshot(amg), never_switched(M1, strong_threshold=0.9))
    host_setup(mi, amg, B)
    assert amg.setup_kind() == (2, 0)
    # a cycle-only setting may change freely
    mi.call("HYPRE_BoomerAMGSetCycleRelaxType", amg.h, 0, 2)
    host_setup(mi, amg, B)
    assert amg.setup_kind() == (2, 0)
    # reason 4: non-Galerkin tolerances, value storage
    for kw in (dict(non_galerkin_tol=0.05), dict(mi_value_storage=2)):
        h = new_amg(mi, name, **kw)
        host_setup(mi, h, B)
        assert h.setup_kind() == (1, 1)
        host_setup(mi, h, B)
        assert h.setup_kind() == (1, 4) and same_hierarchy(rc.snapshot(h), never_switched(M1, **kw))
    # the bad mode
    with pytest.raises(mi.HypreError) as e:
        amg.set_setup_reuse(2)
    assert "returned 4:" in str(e.value)
    mi.call("HYPRE_ClearAllErrors")
    with pytest.raises(mi.HypreError):
        mi.counter("amg_setups_nothing")
    mi.call("HYPRE_ClearAllErrors")


def test_a_failed_setup_leaves_the_handle_not_set_up(mi_lib, oc):
    """a Setup in mode 1 that fails is followed by a rebuild with reason 1.  On the refresh path: a relax type the
    library refuses (a cycle setting, so the verdict is still a refresh) is refused before anything is touched, as a
    full Setup refuses it, and so is relax type 16 in the host-only entry.  On the rebuild path: an interpolation
    type that is not implemented.  (A failure inside the refresh itself needs a smoother: tests/test_gpu_setup_reuse.py.)"""
    mi = mi_lib
    name = "lap7_8"
    M0 = rc.system(oc, name)
    A = host_matrix(mi, M0)
    amg = new_amg(mi, name)
    host_setup(mi, amg, A)
    for bad_relax in (99, 16):
        host_setup(mi, amg, A)
        assert amg.setup_kind() == (2, 0)
        mi.call("HYPRE_BoomerAMGSetCycleRelaxType", amg.h, bad_relax, 1)
        with pytest.raises(mi.HypreError) as e:
            host_setup(mi, amg, A)
        assert "returned 4:" in str(e.value) and "relax_type" in str(e.value)
        mi.call("HYPRE_ClearAllErrors")
        mi.call("HYPRE_BoomerAMGSetCycleRelaxType", amg.h, 8, 1)
        host_setup(mi, amg, A)
        assert amg.setup_kind() == (1, 1)
    host_setup(mi, amg, A)
    assert amg.setup_kind() == (2, 0)
    mi.call("HYPRE_BoomerAMGSetInterpType", amg.h, 99)
    with pytest.raises(mi.HypreError):
        host_setup(mi, amg, A)
    mi.call("HYPRE_ClearAllErrors")
    mi.call("HYPRE_BoomerAMGSetInterpType", amg.h, 6)
    host_setup(mi, amg, A)
    assert amg.setup_kind() == (1, 1)
