"""Value storage of BoomerAMG (HYPRE_MI_BoomerAMGSetValueStorage) on the GPU, in a process of its own so that the
library switches that are read once per process can be varied by the caller (tests/test_gpu_value_storage.py).

    value_storage_worker.py parity SYSTEM N [key=value ...]   mode 1 against mode 2, bit for bit, level by level
    value_storage_worker.py solve  SYSTEM N                   GMRES / BiCGSTAB / FlexGMRES + AMG in modes 0, 1, 2

Every check is an assertion here; the RESULT line carries what the caller compares across processes or gates."""
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from tests.agg2s_common import ij_host, random_mmatrix  # noqa: E402

DIAG_WHICH = (0, 2, 3)


def lap1(n):
    return sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n))


def system(name, n):
    I = sp.identity(n)
    if name == "lap7":
        M = sp.kron(sp.kron(lap1(n), I), I) + sp.kron(sp.kron(I, lap1(n)), I) + sp.kron(sp.kron(I, I), lap1(n))
    elif name == "lap27":
        B = sp.diags([1.0, 1.0, 1.0], [-1, 0, 1], shape=(n, n))
        M = 27.0 * sp.identity(n ** 3) - sp.kron(sp.kron(B, B), B)
    elif name == "arrow":
        # the 7-point operator plus one row and column that touch every unknown weakly: the coarse operators inherit
        # a row longer than a tile (2048 entries)
        M = sp.lil_matrix(system("lap7", n))
        N = M.shape[0]
        M[0, 1:] = M[0, 1:].toarray() - 1e-3
        M[1:, 0] = M[1:, 0].toarray() - 1e-3
        M[0, 0] = 6.0 + 1e-3 * N
        M = M.tocsr()
        M.setdiag(M.diagonal() + 1e-3)
    elif name == "chain":
        # a 1D diffusion operator with a rough coefficient: every coarse operator has about three entries in a row
        c = np.random.default_rng(3).uniform(0.5, 1.5, n + 1)
        M = sp.diags([-c[1:n], c[:n] + c[1:], -c[1:n]], [-1, 0, 1], shape=(n, n))
    elif name == "mm":
        M = random_mmatrix()
    else:
        raise SystemExit("unknown system " + name)
    M = sp.csr_matrix(M)
    M.sort_indices()
    return M


def rounded(a):
    return a.astype(np.float32).astype(np.float64)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def whiches(amg, l):
    return (0, 1) if l == amg.num_levels - 1 else (0, 1, 2, 3, 4, 5)


def storage_report(mi, amg, mode, first_level):
    """kinds per level; asserts that the diag blocks of the levels >= first_level really are of the mode's kind (or
    keep a dictionary) and that mode 1 holds 4 bytes per entry (+ the two pad entries)"""
    rep = []
    for l in range(amg.num_levels):
        row = {}
        for w in whiches(amg, l) + (6, 8):
            kind, nbytes = amg.level_value_storage(l, w)
            nr, nc, nnz = mi.c_int(), mi.c_int(), mi.c_big()
            mi.call("HYPRE_MI_BoomerAMGGetLevelCSRSize", amg.h, l, w, mi.C.byref(nr), mi.C.byref(nc), mi.C.byref(nnz))
            row[w] = kind
            if w in (6, 8) and nr.value == 0:
                continue
            if l < first_level or mode == 0:
                assert kind in (0, 8), (l, w, kind)
            elif w in DIAG_WHICH + (6, 8):
                assert kind in (mode, 8), (l, w, kind, mode)
                if kind == 1:
                    assert nbytes == 4 * (nnz.value + 2), (l, w, nbytes, nnz.value)
                if kind == 2:
                    assert nbytes == 8 * (nnz.value + 2), (l, w, nbytes, nnz.value)
            else:
                assert kind == 2, (l, w, kind)
        rep.append(row)
    return rep


def setup(mi, A, mode, first_level, **kw):
    amg = mi.BoomerAMG(print_level=0, mi_value_storage=mode, mi_value_storage_first_level=first_level, **kw)
    amg.setup(A)
    return amg


def parity(mi, name, n, opts):
    M = system(name, n)
    N = M.shape[0]
    A = mi.matrix_from_scipy(M)
    first_level = int(opts.get("first_level", 1))
    kw = {k: int(v) for k, v in opts.items() if k in ("smooth_type", "smooth_num_levels", "relax_type", "max_levels")}
    if "gs_chunk" in opts:
        mi.call("HYPRE_MI_SetGSChunk", int(opts["gs_chunk"]))
    if "zero_skip" in opts:
        mi.call("HYPRE_MI_SetZeroGuessMode", int(opts["zero_skip"]))
    amgs = {m: setup(mi, A, m, first_level, **kw) for m in (0, 1, 2)}
    a0, a1, a2 = amgs[0], amgs[1], amgs[2]
    nl = a0.num_levels
    assert a1.num_levels == nl and a2.num_levels == nl and nl > first_level, (nl, first_level)
    kinds = {m: storage_report(mi, amgs[m], m, first_level) for m in (0, 1, 2)}
    narrowed = sum(1 for row in kinds[1] for w, k in row.items() if k == 1)
    assert narrowed > 0 and narrowed == sum(1 for row in kinds[2] for w, k in row.items() if k == 2 and w in DIAG_WHICH + (6, 8))

    # the reported hierarchy: mode 0's with rounded values from first_level on, the same from the host-only setup
    Ah = ij_host(mi, M)
    hosts = {}
    for m in (1, 2):
        h = mi.BoomerAMG(print_level=0, mi_value_storage=m, mi_value_storage_first_level=first_level, **kw)
        mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", h.h, Ah.par)
        assert h.num_levels == nl
        hosts[m] = h
    max_rows_l1 = 0
    for l in range(nl):
        for w in whiches(a0, l):
            ia0, ja0, v0, shape = a0.level_csr(l, w)
            if l == 1 and w == 0:
                max_rows_l1 = int(np.diff(ia0).max())
            want = rounded(v0) if l >= first_level else v0
            for m in (1, 2):
                for amg in (amgs[m], hosts[m]):
                    ia, ja, v, sh = amg.level_csr(l, w)
                    assert sh == shape and np.array_equal(ia, ia0) and np.array_equal(ja, ja0), (l, w, m)
                    assert same(v, want), (l, w, m, "device" if amg is amgs[m] else "host-only")
            assert hosts[1].level_value_storage(l, w)[0] == (0 if l < first_level else 1 if w in DIAG_WHICH else 2)

    # relaxation passes and C/F pairs of every level, smoother steps, whole cycles: mode 1 = mode 2, bit for bit
    rng = np.random.default_rng(7)
    names = set()
    pids = [base + l for l in range(1, min(nl, 16)) for base in (mi.PROF_LVL_RESID, mi.PROF_LVL_RELAX, mi.PROF_LVL_RESTRICT,
                                                                mi.PROF_LVL_PROLONG, mi.PROF_LVL_RELAX0)]
    for pid in pids:
        mi.profile_enable(pid, 64)
    def on_mode1(result):
        names.update(mi.profile_kernel_name(pid) for pid in pids)  # the kernels of the call that has just run on a1
        return result

    relax_types = [int(t) for t in opts.get("types", "3,4,6,8,13,14,7,18,11,12").split(",")]
    differs_from_mode0 = 0
    for l in range(nl):
        nrow = a0.level_csr(l, 0)[3][0]
        if nrow == 0:
            continue
        f, u = rng.standard_normal(nrow), rng.standard_normal(nrow)
        last = l == nl - 1
        for t in relax_types:
            for points in ((0,) if last else (0, 1, -1)):
                r1 = on_mode1(a1.relax_level(l, t, points, f, u))
                r2 = a2.relax_level(l, t, points, f, u)
                assert same(r1, r2), ("relax", l, t, points)
                assert np.all(np.isfinite(r1))
                if l >= first_level:
                    differs_from_mode0 += int(not same(r1, a0.relax_level(l, t, points, f, u)))
            if last or t in (7, 18, 11, 12):
                continue
            for first in (1, -1):
                for guess in (None, u):
                    p1 = on_mode1(a1.relax_pair_level(l, t, first, f, guess))
                    assert same(p1, a2.relax_pair_level(l, t, first, f, guess)), ("pair", l, t, first, guess is None)
        if kw.get("smooth_num_levels", 0) > l and not last:
            for guess in (None, u):
                assert same(a1.smooth_level(l, f, guess), a2.smooth_level(l, f, guess)), ("smooth", l, guess is None)
    assert differs_from_mode0 > 0  # the rounded operators are really the ones the passes ran on
    b = mi.IJVector(0, N - 1, rng.standard_normal(N))
    cyc = {}
    for m in (0, 1, 2):
        for zero in (True, False):
            x = mi.IJVector(0, N - 1, np.zeros(N) if zero else np.linspace(-1.0, 1.0, N))
            mi.profile_reset()
            amgs[m].solve(A, b, x)  # max_iterations 1: one V-cycle through every level
            cyc[m, zero] = x.get()
            if m == 1:
                on_mode1(None)
    for zero in (True, False):
        assert same(cyc[1, zero], cyc[2, zero]), ("cycle", zero)
        assert not same(cyc[1, zero], cyc[0, zero])
    row_mapped = mi.c_big()
    mi.call("HYPRE_MI_GetCounter", b"value_storage_row_mapped", mi.C.byref(row_mapped))
    return dict(levels=nl, kinds=kinds[1], kernels=sorted(k for k in names if k), longest_row_l1=max_rows_l1,
                cycle=cyc[1, True].tobytes().hex(), row_mapped_R=row_mapped.value)


def solve(mi, name, n):
    M = system(name, n)
    N = M.shape[0]
    A = mi.matrix_from_scipy(M)
    bvec = np.asarray(M @ np.ones(N))
    out = {}
    for kname, cls in (("gmres", mi.GMRES), ("bicgstab", mi.BiCGSTAB), ("flexgmres", mi.FlexGMRES)):
        tol = 1e-10
        res = {}
        for m in (0, 1, 2):
            amg = mi.BoomerAMG(print_level=0, mi_value_storage=m)
            ks = cls(tolerance=tol, max_iterations=200, kspace=50, print_level=0)
            ks.set_precond(amg)
            b, x = mi.IJVector(0, N - 1, bvec), mi.IJVector(0, N - 1, np.zeros(N))
            ks.setup(A, b, x)
            rc = ks.solve(A, b, x)
            xs = x.get()
            if m:
                assert amg.level_value_storage(1, 0)[0] in (m, 8)
            res[m] = dict(rc=rc, iters=ks.num_iterations, hist=[float(h).hex() for h in ks.residual_history()],
                          true_res=float(np.linalg.norm(bvec - M @ xs) / np.linalg.norm(bvec)))
        out[kname] = dict(tol=tol, modes=res)
    return out


def main():
    what, name, n = sys.argv[1], sys.argv[2], int(sys.argv[3])
    opts = dict(a.split("=", 1) for a in sys.argv[4:])
    mi = ge.load_binding()
    mi.init()
    r = parity(mi, name, n, opts) if what == "parity" else solve(mi, name, n)
    print("RESULT " + json.dumps(r))


if __name__ == "__main__":
    main()
