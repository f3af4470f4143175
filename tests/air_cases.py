"""Operators and markers of the approximate-ideal-restriction / one-point-interpolation tests (tests/test_air_spec.py,
tests/test_gpu_air.py).  Every generator is seeded; what a case is for is asserted by the tests with the restatement
(tests/air_ref.py), not assumed."""
import numpy as np
import scipy.sparse as sp

from tests import systems

VELOCITY = (1.0, 0.6, 0.3)  # x, y, z: times the cell Peclet number
GROUP_LENGTHS = (0, 1, 16, 17, 32, 33, 64)  # both sides of every lane-group boundary of the device solve
FALLBACK_LENGTH = 65


def upwind_constant(n, peclet):
    """7-point diffusion (diag 6, off -1, as tests/systems.py convection_diffusion_3d) plus first-order upwind convection
    with the constant velocity peclet * VELOCITY on the n^3 grid, lexicographic numbering (x fastest): the upstream
    neighbour of direction d takes -peclet * v_d more, the diagonal peclet * v_d."""
    idx = np.arange(n ** 3).reshape(n, n, n)  # [z, y, x]
    rows, cols, vals = [], [], []
    diag = np.full(n ** 3, 6.0)
    for axis, v in ((2, VELOCITY[0]), (1, VELOCITY[1]), (0, VELOCITY[2])):
        for sgn in (-1, +1):
            src, dst = [slice(None)] * 3, [slice(None)] * 3
            if sgn < 0:
                src[axis], dst[axis] = slice(1, None), slice(None, -1)
            else:
                src[axis], dst[axis] = slice(None, -1), slice(1, None)
            r, c = idx[tuple(src)].ravel(), idx[tuple(dst)].ravel()
            rows.append(r)
            cols.append(c)
            vals.append(np.full(len(r), -1.0 - (peclet * v if sgn < 0 else 0.0)))
        diag += peclet * v
    rows.append(idx.ravel())
    cols.append(idx.ravel())
    vals.append(diag)
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n ** 3, n ** 3))
    A.sort_indices()
    return A


def hub_case(lengths, seed, n=700, c_fraction=0.35):
    """An irregular operator (systems.mixed_sign_system) with a seeded marker and planted hub rows, in the manner of
    systems.hub_system: hub number q is a C point whose F-neighbourhood at theta_R = 0.25 has exactly lengths[q]
    points.  Its row holds lengths[q] couplings to seeded F columns (styles go round with q: all -1; all +1; drawn from
    {-1, -0.5, 0.75}: exact ties and both signs), three couplings 0.9 to C columns (above the threshold, but not F), three
    couplings 0.1 to F columns (below it), and a dominant diagonal; every entry of a hub's column is removed from the
    other rows.  One more C row holds its diagonal alone (maximum 0: empty neighbourhood).  Returns (A, cf, hub rows)."""
    rng = np.random.default_rng(seed)
    M = systems.mixed_sign_system(n, seed, .3, .25, 4.5).tolil()
    cf = np.where(rng.random(n) < c_fraction, 1, -1).astype(np.int32)
    special = np.sort(rng.choice(n, size=len(lengths) + 1, replace=False))
    hubs, lone = special[:-1], special[-1]
    cf[special] = 1
    cpts = np.setdiff1d(np.flatnonzero(cf == 1), special)
    fpts = np.flatnonzero(cf == -1)
    M[:, special] = 0.0
    M[special, :] = 0.0
    M[lone, lone] = 3.0
    for q, (h, L) in enumerate(zip(hubs, lengths)):
        pick = rng.choice(fpts, size=L + 3, replace=False)
        strong, weak = pick[:L], pick[L:]
        vals = (-np.ones(L), np.ones(L), rng.choice([-1.0, -0.5, 0.75], size=L))[q % 3]
        if L:
            vals[0] = -1.0 if q % 3 != 1 else 1.0  # the row's maximum is 1 in every style
            M[h, strong] = vals
        M[h, rng.choice(cpts, size=3, replace=False)] = 0.9 if L else 1.0
        M[h, weak] = 0.1
        M[h, h] = 1.01 * L + 4.0
    M = M.tocsr()
    M.eliminate_zeros()
    M.sort_indices()
    return M, cf, hubs


def filter_case():
    """C rows 0, 1, 2 and F points 3 ... 11 whose rows hold their diagonal d alone, so y_t = -a(i, N_t) / d_t: with
    a = -1 row 0 gets y = (1, 0.4, 0.625), row 1 y = (1, 0.8), row 2 y = (1, 0.1, 0.2, 0.25).  At phi = 0.5 row 0 loses
    one entry (some), row 1 none, row 2 all but the largest.  Returns (A, cf)."""
    d = {3: 1.0, 4: 2.5, 5: 1.6, 6: 1.0, 7: 1.25, 8: 1.0, 9: 10.0, 10: 5.0, 11: 4.0}
    M = sp.lil_matrix((12, 12))
    for c, cols in ((0, (3, 4, 5)), (1, (6, 7)), (2, (8, 9, 10, 11))):
        M[c, c] = 4.0
        for j in cols:
            M[c, j] = -1.0
    for j, v in d.items():
        M[j, j] = v
    cf = np.array([1, 1, 1] + [-1] * 9, dtype=np.int32)
    M = M.tocsr()
    M.sort_indices()
    return M, cf


SINGULAR_ROW = 60


def singular_case():
    """A 1-D three-point chain of 60 rows and a gadget of four: i = 60 (diagonal 4; +1 to f1 = 61 and f2 = 62; -0.1 to
    k = 63), f1 (diagonal 2, +1 to f2, -1 to i), f2 (+2 to f1, diagonal 1, -1 to i), k (diagonal 2, -1 to i).  With
    max_row_sum 1 the three others depend strongly on i and nobody on them: PMIS makes i a C point and them F points.
    N_i = {f1, f2} at theta_R = 0.25 (|-0.1| is below 0.25), and the rows of f1 and f2 are (2, 1) and (2, 1) on N_i: the
    elimination meets an exact zero pivot (1 - (1 / 2) * 2).  Returns (A, cf of the gadget rows as Setup leaves it)."""
    n = 64
    M = sp.lil_matrix((n, n))
    for r in range(60):
        M[r, r] = 2.0
        if r > 0:
            M[r, r - 1] = -1.0
        if r < 59:
            M[r, r + 1] = -1.0
    i, f1, f2, k = 60, 61, 62, 63
    M[i, i], M[i, f1], M[i, f2], M[i, k] = 4.0, 1.0, 1.0, -0.1
    M[f1, f1], M[f1, f2], M[f1, i] = 2.0, 1.0, -1.0
    M[f2, f1], M[f2, f2], M[f2, i] = 2.0, 1.0, -1.0
    M[k, k], M[k, i] = 2.0, -1.0
    M = M.tocsr()
    M.sort_indices()
    return M, {i: 1, f1: -1, f2: -1, k: -1}


def fallback_operator(seed=5, n=600, L=FALLBACK_LENGTH):
    """systems.mixed_sign_system with one planted hub h that the library's own PMIS makes a C point with L F neighbours:
    L seeded rows j get the entry (j, h) = -3 * (their largest |coupling|) -- they depend strongly on h, whose measure is
    then above L -- and row h holds (h, j) = -1 for those j, nothing else off the diagonal, and the diagonal 1.01 L.
    Column h is removed from every other row.  Returns (A, h)."""
    rng = np.random.default_rng(seed)
    M = systems.mixed_sign_system(n, seed, 0.0, 0.0, 3.0).tolil()
    h = int(rng.integers(n))
    M[:, h] = 0.0
    M[h, :] = 0.0
    dep = rng.choice(np.setdiff1d(np.arange(n), [h]), size=L, replace=False)
    for j in dep:
        row = M.getrow(j).toarray().ravel()
        off = np.abs(np.delete(row, j)).max()
        M[j, h] = -3.0 * off
        M[j, j] = row[j] + 3.0 * off
    M[h, dep] = -1.0
    M[h, h] = 1.01 * L
    M = M.tocsr()
    M.eliminate_zeros()
    M.sort_indices()
    return M, h


def one_point_case():
    """Six rows for interpolation 100: C points 0, 1, 2; F row 3 with a tie (|a| = 1 to the C points 0 and 2 and 0.5 to 1:
    the lowest column, 0, wins), F row 4 whose strong C entries differ (2 wins with |-2|), F row 5 without a strong C
    point (its only strong neighbour is the F point 4).  Returns (A, strong rows, cf)."""
    M = np.array([[4, -1, 0, -1, 0, 0],
                  [-1, 4, -1, 0, 0, 0],
                  [0, -1, 4, 0, -1, 0],
                  [-1, -.5, -1, 4, 0, 0],
                  [0, -1, -2, 0, 4, -1],
                  [0, 0, 0, 0, -1, 4]], dtype=float)
    strong = [[1, 3], [0, 2], [1, 4], [0, 1, 2], [1, 2, 5], [4]]
    cf = np.array([1, 1, 1, -1, -1, -1], dtype=np.int32)
    return sp.csr_matrix(M), strong, cf


def strong_csr(strong, n):
    indptr = np.cumsum([0] + [len(r) for r in strong])
    indices = np.concatenate([np.asarray(r, dtype=np.int64) for r in strong]) if indptr[-1] else np.zeros(0, dtype=np.int64)
    return sp.csr_matrix((np.ones(indptr[-1]), indices, indptr), shape=(n, n))


# ---- views of a hierarchy and comparisons, shared by the CPU and the GPU tests
def as_csr(parts):
    ia, ja, a, shape = parts
    return sp.csr_matrix((a, ja, ia), shape=shape)


def natural_marker(amg, level):
    """the marker of a level in the level's natural numbering (level_cf reports the C-first renumbered copy)"""
    perm = amg.level_perm(level).astype(np.int64)
    cf = np.empty(len(perm), dtype=np.int32)
    cf[perm] = amg.level_cf(level)
    return cf


def natural_operators(amg, level):
    """(A, cf, P, R) of a level in the natural numbering the hierarchy is built in: rows and columns of the level by its
    own order, coarse rows and columns by the order of the C points; explicit zeros survive"""
    from tests.agg2s_common import csr
    from tests.mm_interp_common import permute_keep_zeros

    perm = amg.level_perm(level).astype(np.int64)       # perm[new] = old
    permc = amg.level_perm(level + 1).astype(np.int64)
    inv, invc = np.empty_like(perm), np.empty_like(permc)
    inv[perm] = np.arange(len(perm))
    invc[permc] = np.arange(len(permc))
    A = csr(amg, level, 0)[inv][:, inv].tocsr()
    A.sort_indices()
    return (A, natural_marker(amg, level), permute_keep_zeros(csr(amg, level, 2), inv, permc),
            permute_keep_zeros(csr(amg, level, 3), invc, perm))


def row_relative_deviation(R, exact):
    """max over the entries of |R.data - exact| / max|row of exact|: every row of R holds a 1, so this is the error of an
    entry against the size of its row (an entry that cancels to nearly 0 is not measured against itself)"""
    exact = np.asarray(exact, dtype=np.longdouble)
    worst = 0.0
    for c in range(R.shape[0]):
        s = slice(R.indptr[c], R.indptr[c + 1])
        worst = max(worst, float(np.abs(R.data[s].astype(np.longdouble) - exact[s]).max() / np.abs(exact[s]).max()))
    return worst


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def same_bits(p, q):
    """two operators as (ia, ja, a, shape): the same pattern and the same bits"""
    return (p[3] == q[3] and np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1])
            and np.array_equal(bits(p[2]), bits(q[2])))


def kernel_cases():
    """name -> (A, cf, theta_R, phi) of the cases the two ...Op entries are compared on: the constant-velocity upwind
    operator with a seeded marker (a third of the points C), the hub operator without and with the filter, the filter
    case.  The hub operator has 259 C rows -- not a multiple of the 256 rows of a workgroup of the per-row kernels, and
    254 of them in the 16-lane class, not a multiple of its 4 rows per workgroup; the filter case has 3, less than one
    workgroup of any kernel."""
    out = {}
    for n in (8, 12):
        for pe in (1000, 0.6):
            cf = np.where(np.random.default_rng(n).random(n ** 3) < 1.0 / 3.0, 1, -1).astype(np.int32)
            out["upwind%d_pe%g" % (n, pe)] = (upwind_constant(n, pe), cf, 0.25, 0.0)
    A, cf, _ = hub_case(GROUP_LENGTHS, 3)
    out["hubs"] = (A, cf, 0.25, 0.0)
    out["hubs_phi0.3"] = (A, cf, 0.25, 0.3)
    A, cf = filter_case()
    out["filter_phi0"] = (A, cf, 0.25, 0.0)
    out["filter_phi0.5"] = (A, cf, 0.25, 0.5)
    return out


def host_cases():
    """kernel_cases() and the cases only the host routine builds: the hub operator with one more hub of 65 F neighbours
    (the neighbourhood the device routine leaves to the host routine), without and with the filter"""
    out = kernel_cases()
    A, cf, _ = hub_case(GROUP_LENGTHS + (FALLBACK_LENGTH,), 3)
    out["hubs65"] = (A, cf, 0.25, 0.0)
    out["hubs65_phi0.3"] = (A, cf, 0.25, 0.3)
    return out
