"""Seeded test systems shared by the parity tests and tests/golden/make_golden.py."""
import numpy as np
import scipy.sparse as sp


def convection_diffusion_3d(n, seed=1234, peclet=0.6):
    """Stand-in for the nalu-wind momentum system of BASELINE.json config 5 (no dump exists offline):
    7-point diffusion (diag 6, off -1) plus first-order UPWIND convection with a seeded, spatially varying
    velocity field -- a diagonally dominant, non-symmetric M-matrix on the n^3 grid, lexicographic numbering."""
    rng = np.random.default_rng(seed)
    N = n ** 3
    idx = np.arange(N).reshape(n, n, n)  # [z, y, x]
    vel = peclet * rng.uniform(-1.0, 1.0, size=(3, n, n, n))  # z, y, x components (cell Peclet numbers)
    rows, cols, vals = [], [], []
    diag = np.full((n, n, n), 6.0)
    for axis in range(3):
        v = vel[axis]
        for sgn in (-1, +1):
            src = [slice(None)] * 3
            dst = [slice(None)] * 3
            if sgn < 0:
                src[axis], dst[axis] = slice(1, None), slice(None, -1)   # neighbour at -1
            else:
                src[axis], dst[axis] = slice(None, -1), slice(1, None)   # neighbour at +1
            r = idx[tuple(src)].ravel()
            c = idx[tuple(dst)].ravel()
            vv = v[tuple(src)].ravel()
            # upwind: flow in +axis direction takes from the -1 neighbour
            conv = np.where(sgn < 0, np.maximum(vv, 0.0), np.maximum(-vv, 0.0))
            rows.append(r)
            cols.append(c)
            vals.append(-1.0 - conv)
        diag += np.abs(v)  # the upwind contributions of both directions sum to |v| on the diagonal
    rows.append(idx.ravel())
    cols.append(idx.ravel())
    vals.append(diag.ravel())
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N))
    A.sort_indices()
    return A


def three_component_rhs(A, seed=99):
    """Three right-hand sides b_c = A x_c with smooth-plus-random exact solutions (component-major (3, N))."""
    rng = np.random.default_rng(seed)
    N = A.shape[0]
    t = np.linspace(0.0, 1.0, N)
    xs = np.stack([1.0 + 0.0 * t, np.sin(6.0 * t) + 0.1 * rng.standard_normal(N), rng.standard_normal(N)])
    return np.stack([A @ x for x in xs]), xs


def mixed_sign_system(n, seed, flip_rows, pos_frac, per, symmetric_pattern=True):
    """An operator that is NOT an M-matrix (sorted CSR): a seeded random pattern of about `per` draws per row
    (symmetrised unless symmetric_pattern=False, so roughly twice as many entries), couplings -|v| - 0.1 of which the
    fraction pos_frac is turned into small positive ones (0.4 |v|), a diagonal that dominates the row by up to 20 %,
    and the fraction flip_rows of the rows multiplied by -1: negative diagonals with positive couplings, the mirrored
    branch of the strength rule, of the interpolation formulas and of the l1 norms."""
    rng = np.random.default_rng(seed)
    B = sp.random(n, n, density=per / n, random_state=rng, format="csr")
    if symmetric_pattern:
        B = (B + B.T).tocsr()
    B = (B - sp.diags(B.diagonal())).tocsr()
    B.eliminate_zeros()
    B.sort_indices()
    B.data = -np.abs(B.data) - 0.1
    pos = rng.random(B.nnz) < pos_frac
    B.data[pos] = 0.4 * np.abs(B.data[pos])
    d = np.asarray(abs(B).sum(axis=1)).ravel() * (1.0 + 0.2 * rng.random(n)) + 1e-3
    flip = rng.random(n) < flip_rows
    M = (sp.diags(np.where(flip, -1.0, 1.0)) @ (B + sp.diags(d))).tocsr()
    M.sort_indices()
    return M


# the operators of the mixed-sign tests: (n, seed, flip_rows, pos_frac, per); 4 to 89 entries per row on average, so
# that the setup kernels pick 4, 8, 16, 32 and 64 lanes per row; the last two are the pure cases (every diagonal
# negative with M-matrix magnitudes; every diagonal positive with 35 % positive couplings)
MIXED_SIGN_CASES = [(2000, 43, .3, .25, 1.5), (2000, 49, .3, .25, 4.5), (2000, 58, .5, .3, 9), (1500, 76, .3, .25, 18),
                    (1200, 130, .3, .25, 45), (2000, 49, 1.0, 0, 4.5), (2000, 49, 0, .35, 4.5)]


# ---- operators of the interpolation-table tests (tests/test_interp_tables_spec.py, tests/test_gpu_interp_tables.py)
HUB_BASE = (3000, 49, .3, .25, 4.5)
HUB_LENGTHS = (16, 17, 32, 33, 128, 129, 512, 513, 1024)   # a table's capacity and one more, for every table


def hub_system(lengths, seed, base=HUB_BASE):
    """mixed_sign_system(*base) with planted ONE-WAY hub rows; returns (operator, hub rows, their lengths).
    Hub number q (row hubs[q], a seeded choice) gets lengths[q] strong couplings to seeded non-hub columns and every entry
    of column hubs[q] is removed from the other rows: nobody depends on a hub, so its PMIS measure stays below 1 and it
    becomes an F point, and no other row's interpolatory set grows.  The style of a hub goes round with q:
      q % 4 == 0   couplings -1, diagonal 1.01 L
      q % 4 == 1   the same row negated (negative diagonal, positive couplings)
      q % 4 == 2   couplings drawn from {-1, -0.5} (both strong at theta <= 0.25: exact ties in |weight|), plus 5 weak
                   couplings +0.25 of the diagonal's sign (terms that go to the diagonal); diagonal 1.01 L + 1.25
      q % 4 == 3   style 2 negated
    so a tuple of lengths repeated four times plants every length in every style."""
    M = mixed_sign_system(*base).tolil()
    n = M.shape[0]
    rng = np.random.default_rng(seed)
    hubs = np.sort(rng.choice(n, size=len(lengths), replace=False))
    others = np.setdiff1d(np.arange(n), hubs)
    M[:, hubs] = 0.0
    M[hubs, :] = 0.0
    for q, (h, L) in enumerate(zip(hubs, lengths)):
        style = q % 4
        cols = rng.choice(others, size=L + (5 if style >= 2 else 0), replace=False)
        vals = -np.ones(L) if style < 2 else -rng.choice([1.0, 0.5], size=L)
        if style >= 2:
            vals = np.concatenate([vals, np.full(5, 0.25)])
        sign = -1.0 if style % 2 else 1.0
        M[h, cols] = sign * vals
        M[h, h] = sign * (1.01 * L + (1.25 if style >= 2 else 0.0))
    M = M.tocsr()
    M.eliminate_zeros()
    M.sort_indices()
    return M, hubs, np.asarray(lengths)


# hubs_ext: under ext+i the bound of a hub is about 1.9 times its length (its own C points plus those of its strong F
# neighbours, with multiplicity).  Lengths and seed were chosen on the CPU so that the bounds hit 128, 129, 512 and 513
# and stay below 1024 on every row (asserted in tests/test_interp_tables_spec.py)
HUB_EXT_LENGTHS = (8, 9, 10, 16, 17, 18, 19, 20) + tuple(range(60, 76)) + tuple(range(256, 288, 2)) + (505, 515, 525, 535)

# name -> (builder arguments of hub_system, or the mixed_sign_system case), strong_threshold, interpolation the
# operator was made for (6 ext+i, 0 classical modified)
INTERP_TABLE_OPERATORS = {
    # dense random operators: hundreds of candidates per row, counted with multiplicity by the bound the kernel bins on
    "dense1200": ((1200, 9, .3, .25, 60), 0.25, 6),
    "dense1600": ((1600, 11, .3, .25, 70), 0.1, 6),
    "hubs": ((HUB_LENGTHS * 4, 7), 0.25, 0),
    "hubs_ext": ((HUB_EXT_LENGTHS, 39), 0.25, 6),
    # one row over the largest table: a hub of 1025 couplings (classical), a hub whose ext+i bound is 1040 (seed chosen so
    # that no row of level 1 exceeds the tables: the coarse levels of the hub operators are dense, and under ext+i most
    # seeds give a level 1 that falls back as well)
    "overflow": ((HUB_LENGTHS * 4 + (1025,), 7), 0.25, 0),
    "overflow_ext": ((HUB_EXT_LENGTHS + (560,), 14), 0.25, 6),
}


def interp_table_operator(name):
    """(operator, hub rows, hub lengths) of a name in INTERP_TABLE_OPERATORS (no hubs: two empty arrays)"""
    args = INTERP_TABLE_OPERATORS[name][0]
    if name.startswith("dense"):
        return mixed_sign_system(*args), np.zeros(0, dtype=int), np.zeros(0, dtype=int)
    return hub_system(*args)
