"""CPU: the value-storage option of BoomerAMG (HYPRE_MI_BoomerAMGSetValueStorage) through the
host-only setup: the hierarchy of mode 1 / mode 2 is mode 0's hierarchy with every stored value v of the levels >=
first_level replaced by (double)(float)v -- numpy's astype(float32).astype(float64) -- and nothing else changed."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.agg2s_common import anisotropic, csr, ij_host, random_mmatrix

FLT_MIN = float(np.finfo(np.float32).tiny)
FLT_MAX = float(np.finfo(np.float32).max)


def _matrix(mi, name):
    if name == "lap7_12":
        return mi.build_laplace_system_host(12, 12, 12, 7, 0, 1)[0]
    if name == "lap27_10":
        return mi.build_laplace_system_host(10, 10, 10, 27, 0, 1)[0]
    if name == "aniso":
        return ij_host(mi, anisotropic())
    return ij_host(mi, random_mmatrix())


def _host_amg(mi, A, mode=None, first_level=1, **kw):
    amg = mi.BoomerAMG(print_level=0, **kw)
    if mode is not None:
        mi.call("HYPRE_MI_BoomerAMGSetValueStorage", amg.h, mode, first_level)
    mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
    return amg


def _rounded(a):
    return a.astype(np.float32).astype(np.float64)


def _fits(a):
    m = np.abs(a[np.isfinite(a) & (a != 0.0)])
    return not (np.any(m > FLT_MAX) or np.any(m < FLT_MIN))


def _whiches(amg, level):
    return (0, 1) if level == amg.num_levels - 1 else (0, 1, 2, 3, 4, 5)


def test_setter_validation(mi_lib):
    mi = mi_lib
    amg = mi.BoomerAMG(print_level=0)
    for mode, first in ((3, 1), (-1, 1), (1, 0), (2, -1)):
        with pytest.raises(mi.HypreError) as e:
            mi.call("HYPRE_MI_BoomerAMGSetValueStorage", amg.h, mode, first)
        assert "value storage" in str(e.value)
        mi.call("HYPRE_ClearAllErrors")
    with pytest.raises(mi.HypreError):
        mi.BoomerAMG(print_level=0, mi_value_storage=7)
    mi.call("HYPRE_ClearAllErrors")
    for mode in (0, 1, 2):
        mi.call("HYPRE_MI_BoomerAMGSetValueStorage", amg.h, mode, 3)


def test_mode0_is_the_hierarchy_as_built(mi_lib, oc):
    """explicit mode 0 = a solver that was never told: every level equals the oracle's, bit for bit, kind 0 everywhere"""
    mi = mi_lib
    A = _matrix(mi, "lap7_12")
    amg = _host_amg(mi, A, mode=0)
    ref = _host_amg(mi, A)
    oamg = oc.Amg(oc.Csr.laplace(12, 12, 12, 7)[0], oc.default_params())
    assert amg.num_levels == ref.num_levels == oamg.num_levels > 2
    for l in range(amg.num_levels):
        oia, oja, oa = oamg.level_A(l).arrays()
        ia, ja, a, _ = amg.level_csr(l, 0)
        assert np.array_equal(ia, oia) and np.array_equal(ja, oja) and np.array_equal(a, oa)
        for w in _whiches(amg, l):
            x, y = amg.level_csr(l, w), ref.level_csr(l, w)
            assert all(np.array_equal(p, q) for p, q in zip(x[:3], y[:3]))
            assert amg.level_value_storage(l, w) == (0, 0)


@pytest.mark.parametrize("first_level", [1, 2])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", ["lap7_12", "lap27_10", "aniso", "randmm"])
def test_rounded_hierarchy(mi_lib, name, mode, first_level):
    mi = mi_lib
    A = _matrix(mi, name)
    ref = _host_amg(mi, A, mode=0)
    amg = _host_amg(mi, A, mode=mode, first_level=first_level)
    assert amg.num_levels == ref.num_levels and amg.num_levels > first_level
    changed = 0
    for l in range(amg.num_levels):
        if l < amg.num_levels - 1:
            assert np.array_equal(amg.level_cf(l), ref.level_cf(l))
        assert np.array_equal(amg.level_perm(l), ref.level_perm(l))
        for w in _whiches(amg, l):
            ia, ja, a, shape = amg.level_csr(l, w)
            ria, rja, ra, rshape = ref.level_csr(l, w)
            assert shape == rshape and np.array_equal(ia, ria) and np.array_equal(ja, rja)
            kind, nbytes = amg.level_value_storage(l, w)
            if l < first_level:
                assert np.array_equal(a, ra) and kind == 0
            else:
                assert np.array_equal(a.view(np.int64), _rounded(ra).view(np.int64))
                # the diag block is what mode 1 narrows; halo blocks keep 8-byte storage holding the rounded values
                assert kind == (mode if w in (0, 2, 3) else 2)
                changed += int(np.count_nonzero(a != ra))
            assert nbytes == 0  # nothing is on the device
    assert changed > 0  # the systems do have values that are not floats below the finest level


def _scaled_mmatrix(mi, target):
    """the M-matrix times a power of two that puts `target` inside the value range of the level-1 operator"""
    M = random_mmatrix()
    ref = _host_amg(mi, ij_host(mi, M), mode=0)
    a1 = np.abs(ref.level_csr(1, 0)[2])
    a1 = a1[a1 != 0.0]
    mid = np.sqrt(a1.min() * a1.max())
    assert a1.min() < 0.5 * mid and a1.max() > 2.0 * mid
    return M * 2.0 ** int(np.round(np.log2(target / mid)))


@pytest.mark.parametrize("target", [FLT_MIN, FLT_MAX])
@pytest.mark.parametrize("mode", [1, 2])
def test_out_of_range_operator_keeps_fp64(mi_lib, mode, target):
    mi = mi_lib
    A = ij_host(mi, _scaled_mmatrix(mi, target))
    ref = _host_amg(mi, A, mode=0)
    amg = _host_amg(mi, A, mode=mode)
    assert amg.num_levels == ref.num_levels > 2
    kept, narrowed = [], []
    for l in range(1, amg.num_levels):
        for op in ((0, 1), (2, 4), (3, 5)):
            if op[0] > 0 and l == amg.num_levels - 1:
                continue
            ra = [ref.level_csr(l, w)[2] for w in op]
            fits = _fits(np.concatenate(ra))  # the rule looks at the operator: both blocks
            for w, r in zip(op, ra):
                a = amg.level_csr(l, w)[2]
                kind = amg.level_value_storage(l, w)[0]
                if fits:
                    assert np.array_equal(a.view(np.int64), _rounded(r).view(np.int64))
                    assert kind == (mode if w == op[0] else 2)
                else:
                    assert np.array_equal(a.view(np.int64), r.view(np.int64)) and kind == 0
            (narrowed if fits else kept).append((l, op[0]))
    assert (1, 0) in kept  # the level-1 operator straddles the limit
    assert any(w in (2, 3) for _, w in narrowed)  # interpolation weights do not scale with the matrix


@pytest.mark.parametrize("name", ["lap7_12", "randmm"])
def test_two_grid_cycle_on_rounded_operators_contracts(mi_lib, name):
    """sanity of the spec: symmetric Gauss-Seidel around the coarse correction, all on the reported rounded level-1
    operators (A_1, P_1, R_1, A_2), is a contraction"""
    mi = mi_lib
    amg = _host_amg(mi, _matrix(mi, name), mode=1)
    assert amg.num_levels > 2
    A1, P1, R1, A2 = (csr(amg, 1, 0).toarray(), csr(amg, 1, 2).toarray(), csr(amg, 1, 3).toarray(),
                      csr(amg, 2, 0).toarray())
    assert np.array_equal(A1, _rounded(A1)) and np.array_equal(P1, _rounded(P1)) and np.array_equal(A2, _rounded(A2))
    I = np.eye(A1.shape[0])
    down = I - np.linalg.solve(np.tril(A1), A1)
    up = I - np.linalg.solve(np.triu(A1), A1)
    K = I - P1 @ np.linalg.solve(A2, R1 @ A1)
    assert float(np.abs(np.linalg.eigvals(up @ K @ down)).max()) < 1.0
