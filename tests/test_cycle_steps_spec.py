"""CPU: the reference and the checkers of tests/cycle_steps_ref.py on hierarchies from the host-only setup.

Each step is evaluated in plain fp64 with the row's products added in seeded shuffled orders -- what a correct kernel may
return.  The checkers must accept every one of those (the reference alone stays inside the bounds) and must reject the
same result with one entry moved by four times its bound (the bounds can fail)."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import cycle_steps_ref as ref
from tests.agg2s_common import ij_host
from tests.systems import convection_diffusion_3d

ORDERS = 3


def _identity_rows(M, every=7):
    """Dirichlet rows kept in the system: rows of P without entries, columns R never reads"""
    M = M.tolil()
    for i in range(0, M.shape[0], every):
        M.rows[i], M.data[i] = [i], [1.0]
    return M.tocsr()


def _hierarchy(mi, name):
    if name == "lap7":
        A, _ = mi.build_laplace_system_host(9, 9, 9, 7, 0, 1)
        kw = {}
    else:
        M = _identity_rows(convection_diffusion_3d(8))
        A = ij_host(mi, M)
        kw = dict(restriction=1, interp_type=100) if name == "air" else {}
    amg = mi.BoomerAMG(print_level=0, **kw)
    mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
    assert amg.num_levels >= 3
    return A, amg


def _moved(x, v, factor=4.0):
    """x with the entry of the largest bound moved by factor times that bound (at least one ulp of the entry)"""
    i = int(np.argmax(v.bound))
    y = x.copy()
    step = max(float(factor * v.bound[i]), 4.0 * np.spacing(abs(y[i])))
    y[i] += step
    return y


@pytest.mark.parametrize("name", ["lap7", "dirichlet", "air"])
def test_checkers_accept_fp64_in_any_order_and_reject_four_bounds(mi_lib, name):
    mi = mi_lib
    keep, amg = _hierarchy(mi, name)
    rng = np.random.default_rng(11)
    empty_p_rows = 0
    for l in range(amg.num_levels - 1):
        A, P, R = (ref.Csr(*amg.level_csr(l, w)) for w in (0, 2, 3))
        n, nn = A.shape[0], P.shape[1]
        assert P.shape == (n, nn) and R.shape == (nn, n)
        empty_p_rows += int((P.m == 0).sum())
        f, u, e = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(nn)
        u[::5] = 0.0
        for o in range(ORDERS):
            order = np.random.default_rng(100 + o)
            r = ref.fp64_rowsums(A, u, order, first=f, sign=-1.0)
            v = ref.check_residual(A, f, u, r)
            assert v and v.ratio < 1.0, (name, l, "residual", v)
            assert not ref.check_residual(A, f, u, _moved(r, v)), (name, l, "residual")
            # the composite path: f - A_FC u_C first, the F columns afterwards
            nc = nn
            t = f.copy()
            C = ref.Csr(*_columns(A, 0, nc))
            F = ref.Csr(*_columns(A, nc, n))
            t[nc:] = ref.fp64_rowsums(C, u, order, first=f, sign=-1.0)[nc:]
            r2 = ref.fp64_rowsums(F, u, order, first=t, sign=-1.0)
            r2[:nc] = r[:nc]
            assert ref.check_residual(A, f, u, r2), (name, l, "composite residual")
            fc = ref.fp64_rowsums(R, r, order)
            v = ref.check_restriction(R, r, fc)
            assert v, (name, l, "restriction", v)
            assert not ref.check_restriction(R, r, _moved(fc, v)), (name, l, "restriction")
            w = ref.fp64_rowsums(P, e, order, first=u)
            v = ref.check_prolongation(P, u, e, w)
            assert v, (name, l, "prolongation", v)
            assert not ref.check_prolongation(P, u, e, _moved(w, v)), (name, l, "prolongation")
            if (P.m == 0).any():  # a row without entries must keep its bits: -0.0 for 0.0 is refused
                i = int(np.flatnonzero(P.m == 0)[0])
                u0 = u.copy()
                u0[i] = -0.0
                w0 = ref.fp64_rowsums(P, e, None, first=u0)
                assert ref.check_prolongation(P, u0, e, w0)
                w0[i] = 0.0
                assert not ref.check_prolongation(P, u0, e, w0)
    assert name == "lap7" or empty_p_rows > 0
    # the collapsed map: a dense n x n matrix applied in fp64, columns in shuffled orders
    n = 37
    B = rng.standard_normal((n, n)) * 10.0 ** rng.integers(-3, 4, size=(n, n))
    f = rng.standard_normal(n)
    for o in range(ORDERS):
        perm = np.random.default_rng(200 + o).permutation(n)
        got = np.zeros(n)
        for j in perm:
            got = got + B[:, j] * f[j]
        v = ref.check_collapsed(B, f, got)
        assert v, v
        assert not ref.check_collapsed(B, f, _moved(got, v))


def _columns(A, lo, hi):
    keep = (A.ja >= lo) & (A.ja < hi)
    M = sp.csr_matrix((A.a[keep], A.ja[keep], np.concatenate([[0], np.cumsum(np.bincount(A.rows[keep], minlength=A.shape[0]))])),
                      shape=A.shape)
    return M.indptr, M.indices, M.data, A.shape


def test_gamma_and_long_double():
    assert np.finfo(ref.LD).nmant >= 63
    assert ref.gamma(1) > ref.LD(2.0 ** -53) and abs(float(ref.gamma(7)) / (7 * 2.0 ** -53) - 1.0) < 1e-14
    # a NaN or an infinity in the result is never inside a bound
    A = ref.Csr([0, 1, 2], [0, 1], [2.0, 3.0], (2, 2))
    assert not ref.check_restriction(A, np.ones(2), np.array([2.0, np.nan]))
    assert not ref.check_restriction(A, np.ones(2), np.array([np.inf, 3.0]))
    assert ref.check_restriction(A, np.ones(2), np.array([2.0, 3.0]))


def test_trace_hooks_declared_and_exported(mi_lib):
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ext = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "HYPRE_mi_ext.h")).read(), flags=re.S)
    for name in ("HYPRE_MI_BoomerAMGTraceCycle", "HYPRE_MI_BoomerAMGGetTraceRecord", "HYPRE_MI_BoomerAMGGetLevelCycleInfo",
                 "HYPRE_MI_BoomerAMGGetCollapsedTail"):
        assert re.search(r"HYPRE_Int\s+%s\s*\(" % name, ext) and hasattr(mi_lib.lib(), name), name
    # a host-only hierarchy has no collapsed tail and reports it
    A, amg = _hierarchy(mi_lib, "lap7")
    assert amg.collapsed_tail() == (-1, None)
    info = amg.level_cycle_info(0)
    assert info["collapsed_level"] == -1 and not info["r_row_mapped"] and info["nc"] == int((amg.level_cf(0) == 1).sum())
