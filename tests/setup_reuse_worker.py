"""Setup reuse on the GPU in a process of its own, for the switches that are read once per process
(tests/test_gpu_setup_reuse.py: MI_HYPRE_DEVICE_SETUP_MIN_ROWS, MI_HYPRE_LOCALITY_ORDER, MI_HYPRE_POISON_ALLOC,
MI_HYPRE_DENSE_TAIL_ROWS).  Modes:
  refresh  device refresh against host-only refresh of the same matrices and changes, every level operator, both
           sub-operators and the three norm arrays bit for bit; the kept structure; reason 6; a digest of everything
  cycle    one cycle of the refreshed hierarchy against the oracle's cycle on the reported levels (default smoother,
           ILU smoother), against a fresh handle (Chebyshev: the oracle has no such smoother); exact scaling by 2^k
  dict     the value format of level 0 follows the values: dictionary, plain, dictionary again
  failed   a zero pivot in a smoother during a refresh: the handle is not set up afterwards
  krylov   GMRES bound to the handle: Setup again refreshes, the solve of the new matrix converges
Prints one RESULT line of JSON."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from tests import ij_cases as cases  # noqa: E402
from tests import ij_update_cases as upd  # noqa: E402
from tests import setup_reuse_cases as rc  # noqa: E402
from tests import setup_reuse_ref as ref  # noqa: E402

CHANGES = ["a", "b8", "b2", "c", "d"]


def device_matrix(mi, M):
    A = cases.new_matrix(mi, 0, M.shape[0] - 1)
    cases.stage(mi, A, [rc.triples(M) + (False,)], True)
    A.assemble()
    return A


def device_update(mi, A, M):
    upd.apply_round(mi, A, [rc.triples(M) + (False,)], device=True)


def host_update(mi, A, M):
    upd.apply_round(mi, A, [rc.triples(M) + (False,)], host_only=True)


def same_hierarchy(x, y):
    return len(x) == len(y) and all(
        all(rc.same_csr(p[k], q[k]) for k in ("A", "P", "R", "Az", "Ar") if k in p) and np.array_equal(p["perm"], q["perm"]) and
        all(rc.same_bits(u, v) for u, v in zip(p["norms"], q["norms"])) and ("cf" not in p or np.array_equal(p["cf"], q["cf"]))
        for p, q in zip(x, y))


def failed_refresh(mi, oc):
    """a refresh that fails inside BoomerAMG::refresh -- the iterative ILU(0) setup of the level-0 smoother meets a zero
    pivot after an update round -- leaves the handle not set up: the next Setup rebuilds with reason 1"""
    M0 = rc.system(oc, "lap7_16")
    Mz = M0.copy()
    Mz.data[Mz.indptr[0] + int(np.where(Mz.indices[Mz.indptr[0]:Mz.indptr[1]] == 0)[0][0])] = 0.0  # a_00 = 0, stored
    A = device_matrix(mi, M0)
    amg = mi.BoomerAMG(print_level=0, setup_reuse=1, smooth_type=5, smooth_num_levels=1, iterative_ilu_algorithm_type=2)
    amg.setup(A)
    amg.setup(A)
    assert amg.setup_kind() == (2, 0)
    device_update(mi, A, Mz)
    message = ""
    try:
        amg.setup(A)
    except mi.HypreError as e:
        message = str(e)
    mi.call("HYPRE_ClearAllErrors")
    device_update(mi, A, M0)
    amg.setup(A)
    kind = amg.setup_kind()
    amg.setup(A)
    return {"message": message, "kind_after_failure": list(kind), "kind_then": list(amg.setup_kind())}


def refresh(mi, oc):
    h = hashlib.sha256()
    out = {"levels": [], "device_levels": []}
    for name in ("lap7_16", "lap27_10"):
        M0 = rc.system(oc, name)
        A = device_matrix(mi, M0)
        Ah = cases.host_only_matrix(mi, M0.shape[0], [rc.triples(M0) + (False,)])
        amg, amgh = mi.BoomerAMG(print_level=0, setup_reuse=1), mi.BoomerAMG(print_level=0, setup_reuse=1)
        amg.setup(A)
        mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amgh.h, Ah.par)
        assert amg.setup_kind() == (1, 1) and amgh.setup_kind() == (1, 1)
        first = rc.snapshot(amg, subs=True)
        out["levels"].append(len(first))
        out["device_levels"].append(sum(1 for l in range(len(first) - 1) if not amg.interp_census(l)["host"]))
        for change in CHANGES:
            M1 = rc.changed(M0, change)
            device_update(mi, A, M1)
            host_update(mi, Ah, M1)
            amg.setup(A)
            mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amgh.h, Ah.par)
            assert amg.setup_kind() == (2, 0) and amgh.setup_kind() == (2, 0), (amg.setup_kind(), amgh.setup_kind())
            dev, host = rc.snapshot(amg, subs=True), rc.snapshot(amgh)
            assert len(dev) == len(host) == len(first)
            for l, (d, g, f) in enumerate(zip(dev, host, first)):
                assert rc.same_csr(d["A"], g["A"]), (name, change, l)
                assert all(rc.same_bits(p, q) for p, q in zip(d["norms"], g["norms"])), (name, change, l)
                assert np.array_equal(d["perm"], f["perm"]) and rc.same_csr(d["A"], f["A"], values=False)
                if "P" in d:
                    assert rc.same_csr(d["P"], f["P"]) and rc.same_csr(d["R"], f["R"]) and np.array_equal(d["cf"], f["cf"])
                Al = ref.csr(*d["A"])
                for w in ("Az", "Ar"):  # entry subsets of A on the kept patterns
                    assert rc.same_csr(d[w], f[w], values=False)
                    if d[w][3][0]:
                        want = ref.lookup_through_permutation(Al, ref.csr(*d[w]))
                        assert None not in want and rc.same_bits(np.array(want), d[w][2]), (name, change, l, w)
                for k in ("A", "Az", "Ar"):
                    h.update(d[k][2].tobytes())
                for v in d["norms"]:
                    h.update(v.tobytes())
            if change == "c":  # level 0 holds the caller's values, level 1 the restatement's bits
                want = ref.lookup_through_permutation(M1, ref.csr(*dev[0]["A"]), dev[0]["perm"], dev[0]["perm"])
                assert rc.same_bits(np.array(want), dev[0]["A"][2])
                vals, fits = ref.triple_product_into_pattern(ref.csr(*dev[0]["A"]), ref.csr(*dev[0]["P"]), ref.csr(*dev[1]["A"]))
                assert fits and rc.same_bits(vals, dev[1]["A"][2])
        # reason 6: the other entry point built the hierarchy; either rebuild has the bits of a handle that never had
        # the switch
        plain_h, plain_d = mi.BoomerAMG(print_level=0), mi.BoomerAMG(print_level=0)
        mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", plain_h.h, A.par)
        plain_d.setup(A)
        assert plain_h.setup_kind() == (1, 0) and plain_d.setup_kind() == (1, 0)
        mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
        assert amg.setup_kind() == (1, 6) and same_hierarchy(rc.snapshot(amg), rc.snapshot(plain_h))
        amg.setup(A)
        assert amg.setup_kind() == (1, 6) and same_hierarchy(rc.snapshot(amg, subs=True), rc.snapshot(plain_d, subs=True))
        amg.setup(A)
        assert amg.setup_kind() == (2, 0)
    out["digest"] = h.hexdigest()
    out["refreshed"] = mi.counter("amg_setups_refreshed")
    return out


def one_cycle(mi, amg, A, f):
    N = len(f)
    fi, ui = mi.IJVector(0, N - 1, f), mi.IJVector(0, N - 1, np.zeros(N))
    amg.solve(A, fi, ui)  # max_iterations 1, tolerance 0: exactly one cycle
    return ui.get()


def cycle(mi, oc):
    name = "lap7_16"
    M0 = rc.system(oc, name)
    M1 = rc.changed(M0, "c")
    N = M0.shape[0]
    f = np.random.default_rng(7).standard_normal(N)
    chunk = mi.c_int()
    mi.call("HYPRE_MI_GetGSChunk", mi.C.byref(chunk))
    out = {}
    for label, kw, okw in (("default", {}, {}), ("ilu", dict(smooth_type=5, smooth_num_levels=1), dict(smooth_type=5, smooth_num_levels=1)),
                           ("cheby", dict(relax_type=16), None)):
        A = device_matrix(mi, M0)
        amg = mi.BoomerAMG(print_level=0, setup_reuse=1, **kw)
        amg.setup(A)
        device_update(mi, A, M1)
        amg.setup(A)
        assert amg.setup_kind() == (2, 0)
        got = one_cycle(mi, amg, A, f)
        if okw is not None:
            snap = rc.snapshot(amg)
            As = [oc.Csr.from_scipy(ref.csr(*d["A"])) for d in snap]
            Ps = [oc.Csr.from_scipy(ref.csr(*d["P"])) for d in snap[:-1]]
            oamg = oc.Amg.from_levels(As, Ps, [d["cf"] for d in snap[:-1]], oc.default_params(gs_chunk=chunk.value, **okw))
            perm = snap[0]["perm"]
            want = np.empty(N)
            want[perm] = oamg.cycle(f[perm])  # the reported levels are in level 0's stored order
        else:
            # the eigenvalue bounds were estimated again: every refreshed level against the restatement of
            # tests/cheby_ref.py, at the tolerance of tests/test_gpu_cheby.py
            from tests import cheby_ref
            from tests.test_cheby_spec import REF_GAP

            gap = 0.0
            for l in range(amg.num_levels):
                have, bd = amg.level_cheby(l), cheby_ref.level_bounds(ref.csr(*amg.level_csr(l, 0)), 10)
                gap = max(gap, max(abs(have[k] - bd[k]) / abs(bd["eig_max"]) for k in bd))
            out["cheby_bounds_gap"], out["cheby_bounds_tol"] = float(gap), max(100.0 * REF_GAP, 1e-13)
            # the cycle against a fresh handle, on 2 A: the fresh interpolation is then the kept one bit for bit, and the
            # operators differ by the rounding of the product's order alone
            M2 = rc.changed(M0, "b2")
            device_update(mi, A, M2)
            amg.setup(A)
            assert amg.setup_kind() == (2, 0)
            got = one_cycle(mi, amg, A, f)
            F = device_matrix(mi, M2)
            fresh = mi.BoomerAMG(print_level=0, **kw)
            fresh.setup(F)
            want = one_cycle(mi, fresh, F, f)
        out[label] = float(np.abs(got - want).max() / np.abs(want).max())
        if label == "default":
            # exact scaling: every operation of the default cycle scales by a power of two exactly
            for k in (1, -3):
                Mk = M1.copy()
                Mk.data *= 2.0 ** k
                device_update(mi, A, Mk)
                amg.setup(A)
                assert amg.setup_kind() == (2, 0)
                scaled = one_cycle(mi, amg, A, f)
                out[f"scaled_{k}"] = bool(rc.same_bits(scaled, got * 2.0 ** -k))
    return out


def dictionary(mi, oc):
    M0 = rc.system(oc, "lap27_16")
    A = device_matrix(mi, M0)
    amg = mi.BoomerAMG(print_level=0, setup_reuse=1)
    amg.setup(A)
    kinds, equal = [amg.level_value_storage(0, 0)[0]], []
    for M in (rc.changed(M0, "d"), M0):
        device_update(mi, A, M)
        amg.setup(A)
        assert amg.setup_kind() == (2, 0)
        kinds.append(amg.level_value_storage(0, 0)[0])
        L0 = amg.level_csr(0, 0)
        perm = amg.level_perm(0)
        want = ref.lookup_through_permutation(M, ref.csr(*L0), perm, perm)
        equal.append(bool(None not in want and rc.same_bits(np.array(want), L0[2])))
    return {"kinds": kinds, "equal": equal}


def krylov(mi, oc):
    out = {}
    for name in ("lap7_16", "lap27_10"):
        M0 = rc.system(oc, name)
        M1 = rc.changed(M0, "c")
        N = M0.shape[0]
        bv = np.cos(np.arange(N, dtype=np.float64))
        A = device_matrix(mi, M0)
        b, x = mi.IJVector(0, N - 1, bv), mi.IJVector(0, N - 1, np.zeros(N))
        amg = mi.BoomerAMG(print_level=0, setup_reuse=1)
        gm = mi.GMRES(tolerance=1e-9, max_iterations=100, kspace=20, print_level=0)
        gm.set_precond(amg)
        gm.setup(A, b, x)
        device_update(mi, A, M1)
        gm.setup(A, b, x)
        assert amg.setup_kind() == (2, 0)
        assert gm.solve(A, b, x) == 0
        rel = float(np.linalg.norm(bv - M1 @ x.get()) / np.linalg.norm(bv))
        F = device_matrix(mi, M1)
        xf = mi.IJVector(0, N - 1, np.zeros(N))
        amg2 = mi.BoomerAMG(print_level=0)
        gm2 = mi.GMRES(tolerance=1e-9, max_iterations=100, kspace=20, print_level=0)
        gm2.set_precond(amg2)
        gm2.setup(F, b, xf)
        assert gm2.solve(F, b, xf) == 0
        out[name] = {"true_rel_res": rel, "iters_refreshed": gm.num_iterations, "iters_fresh": gm2.num_iterations}
    return out


def main():
    mi = ge.load_binding()
    oc = ge.load_oracle()
    mi.init()
    fn = {"refresh": refresh, "cycle": cycle, "dict": dictionary, "krylov": krylov, "failed": failed_refresh}[sys.argv[1]]
    print("RESULT " + json.dumps(fn(mi, oc)))


if __name__ == "__main__":
    main()
