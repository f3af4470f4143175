"""Operators with at most 256 distinct values (bit patterns) for the value-dictionary kernels: spmv_stream_xc<*, *, true, *>
and gs_tile_k<true, *> (kernels.hip, k::build_value_dictionary).  CPU only, seeded; every generator returns a scipy CSR
matrix with sorted indices, so that stored position k of the device block is entry k of `.data`.

The dictionary is built for operators with an x cache (mean row length >= 3), nnz >= 65536 and at most 256 distinct values
in a sample of 65536 entries taken at stride nnz // 65536; an entry outside the sample's table refuses it afterwards.

tests/test_value_dictionary_spec.py checks what is claimed here; tests/test_gpu_value_dictionary.py runs the kernels."""
import numpy as np
import scipy.sparse as sp

THRESHOLD = 1 << 16  # entries from which an operator gets a dictionary, and the size of the sample

STRIDES = {"rowlen7": 3, "rowlen17": 8, "rowlen33": 16, "rowlen65": 32, "rowlen93": 46}  # rows couple to i +- 64 m
LPR = {"rowlen7": 1, "rowlen17": 2, "rowlen33": 4, "rowlen65": 8, "rowlen93": 8}  # lanes per row of the 2048-entry tiles
PLANT_EVERY = 97  # rows i, i + 1 with one weak coupling: neighbours in the C-first ordering too -> coupled chunks

SEED = 5
# name -> (kind, rows, distinct values): the relaxation cases (M-matrices).  Rows: the smallest count, not a multiple of 8,
# with 65536 entries -- for rowlen65 / rowlen93 the smallest that leaves a thousand rows of full length between the two
# ends of the band, where the tiles hold at most 32 rows (8 lanes per row).  `scattered` is not asked for by a threshold:
# its tiles hold more than 1024 unique columns, which the plain tile kernel gathers in two batches and the dictionary
# one in one.
RELAX = {"rowlen7": ("rowlen7", 9445, 16), "rowlen17": ("rowlen17", 4122, 64), "rowlen33": ("rowlen33", 2521, 130),
         "rowlen65": ("rowlen65", 6001, 256), "rowlen93": ("rowlen93", 7001, 200), "ragged": ("ragged", 8892, 255),
         "wide": ("wide", 469, 256), "scattered": ("scattered", 20001, 100)}
# zero-guess pairs: the level operator with zero_from (mode 1), the zero-guess sub-operator (mode 3).  The sub-operator of
# the rowlen kinds has 2.4 entries per row whatever the size (few C points, and an F row keeps only its C columns and its
# chunk): no x cache, hence no dictionary.  The one of `ragged` has 4.2, and 65536 entries from 16 000 rows on.
ZERO = {"rowlen17-12003": ("rowlen17", 12003, 64), "rowlen65": RELAX["rowlen65"], "ragged-16001": ("ragged", 16001, 255)}
# SpMV only: every entry from the palette of both signs
SPMV = {"ragged": ("ragged", 9101, 200), "rowlen33": ("rowlen33", 2521, 130), "wide": ("wide", 469, 256),
        "scattered": ("scattered", 20001, 100)}
GIANT = {"giant-ragged": ("ragged", 9101, 64, 3000), "giant-wide": ("wide", 5003, 256, 5000)}
REFUSALS = ("distinct257", "tail_miss", "stride_miss", "below_threshold", "at_threshold", "distinct256")
RAGGED_STREAM_ROWS = 10001


def relax_case(name):
    kind, n, nd = (RELAX.get(name) or ZERO[name])
    return palette_operator(kind, n, nd, SEED)


def spmv_case(name):
    """(M, info) of an SpMV case: SPMV, GIANT or REFUSALS; info["kind"] is the value kind the device must report"""
    if name in SPMV:
        kind, n, nd = SPMV[name]
        return palette_operator(kind, n, nd, SEED, mmatrix=False, empty_rows=(kind == "ragged")), dict(kind=8, extra=None)
    if name in GIANT:
        kind, n, nd, length = GIANT[name]
        return giant_operator(kind, n, nd, SEED, length), dict(kind=8, extra=None, giant=length)
    return refusal_case(name)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def distinct(M):
    """number of distinct stored values, as the dictionary counts them: by bit pattern"""
    return len(np.unique(bits(M.data)))


def mixed_palette(m):
    """m distinct doubles of both signs, four in five of them no floats: -0.1, 0.2, -0.3, ...  (the table is sorted by the signed
    64-bit pattern: the negative values by rising magnitude, then the positive ones)"""
    k = np.arange(1, m + 1)
    return 0.1 * k * np.where(k % 2 == 1, -1.0, 1.0)


def negative_palette(m):
    """m distinct doubles in [-1.2, -0.8): -0.1 k for fractional k; all strong couplings at the default threshold"""
    return -0.1 * (8.0 + 4.0 * np.arange(m) / m)


def _draw(rng, count, m):
    """palette indices of `count` entries, every one of the m occurring"""
    assert count >= m
    idx = rng.integers(0, m, count)
    idx[rng.permutation(count)[:m]] = np.arange(m)
    return idx


def _pairs(kind, n, rng):
    """(lo, hi, weak): the symmetric pattern's pairs lo < hi, and which of them are planted weak couplings"""
    i = np.arange(n)
    if kind in STRIDES:
        assert n > 128 * STRIDES[kind], "no row would have its full length"
        lo = np.concatenate([i[: n - 64 * m] for m in range(1, STRIDES[kind] + 1)])
        hi = np.concatenate([i[: n - 64 * m] + 64 * m for m in range(1, STRIDES[kind] + 1)])
        p = np.arange(40, n - 1, PLANT_EVERY)
        weak = np.r_[np.zeros(len(lo), dtype=bool), np.ones(len(p), dtype=bool)]
        return np.r_[lo, p], np.r_[hi, p + 1], weak
    if kind == "ragged":
        # 0..12 off-diagonal entries: the pairs (i, i + o) of six offsets, each kept with probability 0.6; rows = 0 mod 17
        # keep none
        lo, hi = [], []
        for o in (1, 2, 3, 5, 8, 13):
            keep = rng.random(n - o) < 0.6
            lo.append(i[: n - o][keep])
            hi.append(i[: n - o][keep] + o)
        lo, hi = np.concatenate(lo), np.concatenate(hi)
        keep = (lo % 17 != 0) & (hi % 17 != 0)
        lo, hi = lo[keep], hi[keep]
    elif kind == "wide":
        # 100..300 entries: the 300 rows within a cyclic distance of 150, each pair kept with probability 0.47
        lo, hi = [], []
        for o in range(1, 151):
            keep = rng.random(n) < 0.47
            a, b = i[keep], (i[keep] + o) % n
            lo.append(np.minimum(a, b))
            hi.append(np.maximum(a, b))
        lo, hi = np.concatenate(lo), np.concatenate(hi)
    elif kind == "scattered":
        # about 8 off-diagonal entries: four partners per row, uniform over all rows
        a = np.repeat(i, 4)
        b = rng.integers(0, n, len(a))
        keep = a != b
        lo, hi = np.minimum(a, b)[keep], np.maximum(a, b)[keep]
        key = np.unique(lo.astype(np.int64) * n + hi)
        lo, hi = (key // n).astype(np.int64), (key % n).astype(np.int64)
    else:
        raise ValueError("unknown kind " + kind)
    return lo, hi, np.zeros(len(lo), dtype=bool)


def _assemble(n, rows, cols, vals):
    M = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    M.sort_indices()
    assert M.has_canonical_format
    return M


def _pow2_diagonal(n, rows, vals):
    """the next power of two at or above 1.01 x the absolute row sum (1 for a row without off-diagonals)"""
    s = np.bincount(rows, weights=np.abs(vals), minlength=n)
    return np.where(s > 0.0, 2.0 ** np.ceil(np.log2(np.maximum(1.01 * s, 1e-300))), 1.0)


def palette_operator(kind, n, ndistinct, seed, mmatrix=True, empty_rows=False):
    """An operator of the row-length kind with exactly `ndistinct` distinct stored values.

    mmatrix (the relaxation cases): symmetric M-matrix; the off-diagonals come from negative_palette (planted weak
    couplings of the rowlen kinds are -1e-3), the diagonal is the next power of two at or above 1.01 x the absolute row
    sum, so it takes a handful of values and the table holds both signs.
    not mmatrix (SpMV only): the same pattern, every stored entry -- the diagonal too -- from mixed_palette(ndistinct);
    empty_rows drops the diagonal of the rows without off-diagonals, which are then truly empty."""
    rng = np.random.default_rng(seed)
    lo, hi, weak = _pairs(kind, n, rng)
    rows, cols = np.r_[lo, hi], np.r_[hi, lo]
    d = np.arange(n)
    if not mmatrix:
        if empty_rows:
            d = d[np.bincount(rows, minlength=n) > 0]
        pal = mixed_palette(ndistinct)
        idx = _draw(rng, len(lo), ndistinct)
        M = _assemble(n, np.r_[rows, d], np.r_[cols, d], np.r_[pal[idx], pal[idx], pal[_draw(rng, len(d), ndistinct)]])
        assert distinct(M) == ndistinct
        return M
    # the diagonal's values depend (slightly) on the palette's size and the other way round: settle the two
    extra = 1 if weak.any() else 0
    m = ndistinct - extra - 4
    draw_seed = rng.integers(1 << 30)
    for _ in range(8):
        assert m >= 1
        r2 = np.random.default_rng(draw_seed)
        w = np.full(len(lo), -1e-3)
        w[~weak] = negative_palette(m)[_draw(r2, int((~weak).sum()), m)]
        vals = np.r_[w, w]
        diag = _pow2_diagonal(n, rows, vals)
        total = m + extra + len(np.unique(diag))
        if total == ndistinct:
            break
        m += ndistinct - total
    M = _assemble(n, np.r_[rows, d], np.r_[cols, d], np.r_[vals, diag])
    assert distinct(M) == ndistinct, (distinct(M), ndistinct)
    return M


def giant_operator(base, n, ndistinct, seed, length):
    """SpMV only: the `ragged` (with truly empty rows) or `wide` operator plus one row of `length` entries, longer than
    its tile (2048 entries, 4096 for the wide one), in the middle of the matrix."""
    M = palette_operator(base, n, ndistinct, seed, mmatrix=False, empty_rows=(base == "ragged")).tolil()
    rng = np.random.default_rng(seed + 1)
    r = n // 2 + 3
    cols = np.sort(rng.choice(n, size=length, replace=False))
    pal = mixed_palette(ndistinct)
    M.rows[r] = [int(c) for c in cols]
    M.data[r] = [float(v) for v in pal[rng.integers(0, ndistinct, length)]]
    M = M.tocsr()
    M.sort_indices()
    assert distinct(M) == ndistinct and np.diff(M.indptr)[r] == length
    return M


def _ragged_stream(n, seed, nnz=None):
    """pattern of the SpMV-only `ragged` operator (truly empty rows), cut after `nnz` stored entries when given: the
    rows behind the cut are empty"""
    M = palette_operator("ragged", n, 2, seed, mmatrix=False, empty_rows=True)
    if nnz is not None:
        assert M.nnz >= nnz
        ia = np.minimum(M.indptr, nnz)
        M = sp.csr_matrix((M.data[:nnz], M.indices[:nnz], ia), shape=M.shape)
    return M


def refusal_case(name, seed=11):
    """(M, info) for the routes of k::build_value_dictionary; info: kind (the value kind the device must report: 8
    dictionary, 0 plain stream), extra (the value that forces the outcome, or None) and the stored positions the GPU test
    asserts on the device's own arrays.

      distinct257      257 values, all of them among the first 65536 entries: refused before anything is encoded
      tail_miss        65536 < nnz < 131072 (sample: entries 0..65535 at stride 1): 20 values, a 21st only behind them
      stride_miss      131072 <= nnz < 196608 (stride 2: the even positions): 20 values, a 21st only at odd positions
      at_threshold     nnz = 65536 exactly: accepted
      below_threshold  the same operator without its last entry, nnz = 65535: no dictionary
      distinct256      256 values: accepted, and table index 255 (the largest positive value) occurs at an odd and at an
                       even position"""
    rng = np.random.default_rng(seed)
    if name in ("at_threshold", "below_threshold"):
        M = _ragged_stream(RAGGED_STREAM_ROWS, seed, THRESHOLD - (name == "below_threshold"))
        M.data[:] = mixed_palette(40)[_draw(np.random.default_rng(seed + 2), THRESHOLD, 40)][: M.nnz]
        return M, dict(kind=8 if name == "at_threshold" else 0, extra=None)
    n = 20001 if name == "stride_miss" else RAGGED_STREAM_ROWS
    M = _ragged_stream(n, seed)
    nnz = M.nnz
    if name == "distinct257":
        M.data[:] = mixed_palette(257)[_draw(rng, nnz, 257)]
        M.data[:257] = mixed_palette(257)
        return M, dict(kind=0, extra=None)
    if name == "distinct256":
        pal = mixed_palette(256)
        M.data[:] = pal[_draw(rng, nnz, 256)]
        top = pal[np.argmax(bits(pal))]
        M.data[[1000, 1001, nnz - 2, nnz - 1]] = top
        return M, dict(kind=8, extra=None, top=float(top))
    extra = 77.7
    M.data[:] = mixed_palette(20)[_draw(rng, nnz, 20)]
    if name == "tail_miss":
        assert THRESHOLD < nnz < 2 * THRESHOLD
        M.data[[THRESHOLD, nnz - 3]] = extra  # the first position behind the sample, and one near the end
    elif name == "stride_miss":
        assert 2 * THRESHOLD <= nnz < 3 * THRESHOLD
        M.data[[1, 70001, 2 * THRESHOLD - 1]] = extra  # odd positions, one of them the last before the sample's end
    else:
        raise ValueError("unknown case " + name)
    return M, dict(kind=0, extra=extra)


def sample_positions(nnz):
    """the stored positions k::build_value_dictionary looks at before it encodes"""
    sample = min(nnz, THRESHOLD)
    return np.arange(sample) * (nnz // sample)


def rounded(M):
    """the operator fp32 value storage holds: every value through float"""
    R = M.copy()
    R.data = R.data.astype(np.float32).astype(np.float64)
    return R


# ---------------------------------------------------------------- reference
def reference_matvec(M, x, alpha=1.0, beta=0.0, b=None):
    """alpha A x + beta b in long double, row by row, and the bound of the fp64 result of ANY summation order:

        |y_i - ref_i| <= (L_i + 3) 2^-53 (|alpha| (|A||x|)_i + |beta b_i|),      L_i = entries of row i

    (L_i products and L_i - 1 additions in some order: (1 + u)^L_i; the scaling by alpha, by beta and the final addition:
    three more roundings; the long double's own error is 2^-11 of that.)  Returns (ref, bound), both long double."""
    M = M.tocsr()
    n = M.shape[0]
    ld = np.longdouble
    rows = np.repeat(np.arange(n), np.diff(M.indptr))
    prod = M.data.astype(ld) * np.asarray(x, dtype=np.float64).astype(ld)[M.indices]
    ax, absax = np.zeros(n, dtype=ld), np.zeros(n, dtype=ld)
    np.add.at(ax, rows, prod)
    np.add.at(absax, rows, np.abs(prod))
    bb = np.zeros(n, dtype=ld) if b is None else np.asarray(b, dtype=np.float64).astype(ld)
    ref = ld(alpha) * ax + ld(beta) * bb
    bound = (np.diff(M.indptr) + 3).astype(ld) * ld(2.0) ** -53 * (abs(ld(alpha)) * absax + np.abs(ld(beta) * bb))
    return ref, bound


# ---------------------------------------------------------------- launch geometry, restated
def tile_schedule(indptr):
    """Row ranges of the tiles of an operator that the tile Gauss-Seidel kernel may sweep (k::build_row_blocks restated):
    whole 8-row chunks while the tile stays below 2048 entries and within 256 rows -- 4096 entries and 512 rows for a mean
    row length of 100 or more -- never across a multiple of 8192 rows; row by row where not even one chunk fits, and a row
    longer than a tile alone.  Returns (rb, tile_entries, block)."""
    ia = np.asarray(indptr, dtype=np.int64)
    n = len(ia) - 1
    tile, block = (4096, 512) if n > 0 and ia[n] / n >= 100.0 else (2048, 256)
    rb, r = [0], 0
    while r < n:
        limit = min(n, (r // 8192 + 1) * 8192)
        e = r
        if r % 8 == 0:
            while e < limit and e - r < block:
                e2 = min(e + 8, limit)
                if ia[e2] - ia[r] > tile - 1:
                    break
                e = e2
        if e == r:
            while e < limit and e - r < block and ia[e + 1] - ia[r] <= tile - 1:
                e += 1
            e = max(e, r + 1)
        rb.append(e)
        r = e
    return np.array(rb), tile, block


def tile_census(M):
    """per tile of the operator: rows, lanes per row of gs_tile_k, entries, unique columns"""
    M = M.tocsr()
    rb, tile, block = tile_schedule(M.indptr)
    nr = np.diff(rb)
    lpr = np.where(nr <= block // 8, 8, np.where(nr <= block // 4, 4, np.where(nr <= block // 2, 2, 1)))
    entries = M.indptr[rb[1:]] - M.indptr[rb[:-1]]
    uniq = np.array([len(np.unique(M.indices[M.indptr[a]:M.indptr[b]])) for a, b in zip(rb[:-1], rb[1:])])
    return dict(rb=rb, tile=tile, block=block, rows=nr, lpr=lpr, entries=entries, unique=uniq)


# ---------------------------------------------------------------- a coarse level with a dictionary
PENDANT = {"rowlen17": ("rowlen17", 4122, 64), "wide": ("wide", 469, 200)}  # S: (kind, rows, distinct values)


def pendant_operator(name):
    """(M, A1): a fine operator whose FIRST COARSE level is known in advance and has few distinct values -- fp32 value
    storage starts at level 1 (level 0 is never narrowed), and Galerkin operators otherwise hold thousands of values.

    M = [[S', -4 E], [-4 E^T, 8 I]]: S is the palette operator of the kind on rows 0..ns-1, and every row c of it has two
    pendant rows ns + 2c, ns + 2c + 1 coupled to nothing but c.  In a row of S' the couplings inside S (0.8 .. 1.2) are weak
    beside the two of 4, so the strength graph is a set of stars: their centres become the C points, the pendants F
    points that interpolate from their centre with weight 4 / 8.  Then level 1 is A1 = S' - 4 I exactly (every product and
    sum in P^T M P is exact: powers of two times one value): S's off-diagonals and a diagonal of a few small integers."""
    kind, ns, nd = PENDANT[name]
    S = palette_operator(kind, ns, nd, SEED).tocsr()
    off = (S - sp.diags(S.diagonal())).tocsr()
    off.eliminate_zeros()
    rowsum = np.abs(off).sum(axis=1).A1 + 8.0
    S1 = (off + sp.diags(2.0 ** np.ceil(np.log2(1.01 * rowsum)))).tocsr()
    c = np.repeat(np.arange(ns), 2)
    E = sp.csr_matrix((np.full(2 * ns, -4.0), (c, np.arange(2 * ns))), shape=(ns, 2 * ns))
    M = sp.bmat([[S1, E], [E.T, 8.0 * sp.identity(2 * ns)]]).tocsr()
    M.sort_indices()
    A1 = (S1 - 4.0 * sp.identity(ns)).tocsr()
    A1.sort_indices()
    return M, A1
