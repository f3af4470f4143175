"""Inputs and helpers of the IJ assembly tests (test_ij_assembly_spec.py on the CPU, test_gpu_ij_device_assembly.py and
its workers on the GPU).  A batch is (rows, cols, vals, add): one SetValues2 / AddToValues2 call with one entry per row
id, global ids.  fold() is the specification of HYPRE_IJMatrixAssemble in plain Python, written for these tests: a
dict keyed by (row, column), walked in submission order."""
import ctypes as C

import numpy as np

BIG = 1e16


def fold(batches, ilower, iupper, jlower, jupper):
    """-> ((ia, ja, a) of the diag block with local columns, (ia, global columns, a) of the rest), columns ascending.
    First occurrence of a pair: the value as it is; later: Set replaces, Add adds with a plain +."""
    run = {}
    for rows, cols, vals, add in batches:
        for r, c, v in zip(rows.tolist(), cols.tolist(), vals):
            key = (r, c)
            if key not in run:
                run[key] = np.float64(v)
            elif add:
                run[key] = np.float64(run[key] + np.float64(v))
            else:
                run[key] = np.float64(v)
    n = iupper - ilower + 1
    dia, oia = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
    dja, da, oj, oa = [], [], [], []
    for r, c in sorted(run):
        assert ilower <= r <= iupper
        if jlower <= c <= jupper:
            dia[r - ilower + 1] += 1
            dja.append(c - jlower)
            da.append(run[(r, c)])
        else:
            oia[r - ilower + 1] += 1
            oj.append(c)
            oa.append(run[(r, c)])
    return ((np.cumsum(dia), np.array(dja, dtype=np.int32), np.array(da, dtype=np.float64)),
            (np.cumsum(oia), np.array(oj, dtype=np.int64), np.array(oa, dtype=np.float64)))


def duplicates_small():
    """Three batches (Set, Add, Set) on 40 rows x 40 columns: pairs occur 1-4 times, sums that depend on the
    association (1e16, 1, -1e16), an explicit zero, an empty row (17), unsorted rows."""
    rng = np.random.default_rng(20261017)
    n = 40
    ent = [[], [], []]
    for r in range(n):
        if r == 17:
            continue
        for c in rng.choice(n, size=int(rng.integers(1, 7)), replace=False):
            for _ in range(int(rng.integers(1, 5))):
                v = float(rng.choice([BIG, 1.0, -BIG, 0.5, 3.0, -2.25, 1e-3]))
                ent[int(rng.integers(0, 3))].append((r, int(c), v))
    for b in ent:
        order = rng.permutation(len(b))
        b[:] = [b[i] for i in order]
    # row 17 stays empty; row 3 / column 3 is built by hand after removing what the draw put there
    for b in ent:
        b[:] = [e for e in b if not (e[0] == 3 and e[1] in (3, 4, 5)) and not (e[0] == 9 and e[1] == 9)]
    ent[0].append((3, 3, 0.0))                                           # Set 0, then added to: (0 + 1e16 + 1) - 1e16 = 0
    ent[1] += [(3, 3, BIG), (3, 3, 1.0), (3, 3, -BIG)]
    ent[1] += [(3, 4, BIG), (3, 4, -BIG), (3, 4, 1.0)]                    # first occurrence in an Add batch: (1e16 - 1e16) + 1 = 1
    ent[0].append((3, 5, 7.0))
    ent[1].append((3, 5, 1.0))
    ent[2].append((3, 5, -4.0))                                          # a later Set replaces the sum
    ent[0].append((9, 9, 0.0))                                           # an explicit zero stays
    out = []
    for b, add in zip(ent, (False, True, False)):
        a = np.array(b, dtype=np.float64).reshape(-1, 3)
        out.append((a[:, 0].astype(np.int64), a[:, 1].astype(np.int64), np.ascontiguousarray(a[:, 2]), add))
    return n, out


def duplicates_large(nrows=2000, seed=7):
    """2000 rows of 1-30 distinct columns, every pair repeated up to 4 times across three batches (Set, Add, Set)."""
    rng = np.random.default_rng(seed)
    rr, cc = [], []
    for r in range(nrows):
        k = int(rng.integers(1, 31))
        cols = rng.choice(nrows, size=k, replace=False)
        rep = rng.integers(1, 5, size=k)
        cc.append(np.repeat(cols, rep))
        rr.append(np.full(int(rep.sum()), r))
    rr, cc = np.concatenate(rr).astype(np.int64), np.concatenate(cc).astype(np.int64)
    vv = rng.choice([BIG, 1.0, -BIG, 0.5, 3.0, -2.25, 0.0], size=len(rr))
    which = rng.integers(0, 3, size=len(rr))
    out = []
    for b, add in enumerate((False, True, False)):
        idx = rng.permutation(np.nonzero(which == b)[0])
        out.append((rr[idx].copy(), cc[idx].copy(), vv[idx].copy(), add))
    return nrows, out


def ragged(long_len=10000, ncols=12000, seed=11):
    """12 000 x 12 000: mostly empty rows, single-entry rows, and row 5000 with long_len unsorted entries on 6000
    distinct columns (duplicates), from a Set batch followed by an Add batch."""
    rng = np.random.default_rng(seed)
    single = np.arange(0, ncols, 7, dtype=np.int64)
    single = single[single != 5000]
    lc = rng.integers(0, 6000, size=long_len).astype(np.int64) * 2
    rows = np.concatenate([single, np.full(long_len, 5000, dtype=np.int64)])
    cols = np.concatenate([(single * 5) % ncols, lc])
    vals = rng.choice([BIG, 1.0, -BIG, 0.5, 3.0], size=len(rows))
    p = rng.permutation(len(rows))
    rows, cols, vals = rows[p], cols[p], vals[p]
    h = len(rows) // 2
    return ncols, [(rows[:h].copy(), cols[:h].copy(), vals[:h].copy(), False),
                   (rows[h:].copy(), cols[h:].copy(), vals[h:].copy(), True)]


def laplace_triples(mi, n, stencil, ilower=None, iupper=None):
    """(rows, cols, vals) of the library's host generator as numpy arrays, in row order"""
    N = n ** 3
    ilower = 0 if ilower is None else ilower
    iupper = N - 1 if iupper is None else iupper
    g = mi.laplace3d(n, n, n, stencil, ilower, iupper)
    nnz = g["nnz"]
    as_np = lambda p, t, dt: np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), shape=(max(nnz, 1),)).copy()[:nnz].astype(dt)
    out = (as_np(g["rows"], mi.c_big, np.int64), as_np(g["cols"], mi.c_big, np.int64), as_np(g["vals"], mi.c_dbl, np.float64))
    mi.laplace3d_free(g)
    return out


def new_matrix(mi, ilower, iupper, jlower=None, jupper=None, device=True):
    """IJMatrix; device=False leaves out HYPRE_IJMatrixInitialize, which needs a GPU (host-only assembly)"""
    if device:
        return mi.IJMatrix(ilower, iupper, jlower, jupper)
    jlower = ilower if jlower is None else jlower
    jupper = iupper if jupper is None else jupper
    A = mi.IJMatrix.__new__(mi.IJMatrix)
    A.h = mi.vp()
    A.ilower, A.iupper = ilower, iupper
    mi.call("HYPRE_IJMatrixCreate", 0, mi.c_big(ilower), mi.c_big(iupper), mi.c_big(jlower), mi.c_big(jupper), C.byref(A.h))
    mi.call("HYPRE_IJMatrixSetObjectType", A.h, mi.HYPRE_PARCSR)
    A.par = mi.vp()
    mi.call("HYPRE_IJMatrixGetObject", A.h, C.byref(A.par))
    return A


def host_only_matrix(mi, n, batches):
    A = new_matrix(mi, 0, n - 1, device=False)
    for rows, cols, vals, add in batches:
        A.set_values_coo(rows, cols, vals, add=add)
    mi.call("HYPRE_MI_IJMatrixAssembleHostOnly", A.h)
    return A


def stage(mi, A, batches, device, keep=None):
    """hand the batches to A: numpy arrays (the host path) or torch CUDA tensors by address (device=True); keep
    collects the tensors so that the caller can overwrite them"""
    if not device:
        for rows, cols, vals, add in batches:
            A.set_values_coo(rows, cols, vals, add=add)
        return
    import torch

    for rows, cols, vals, add in batches:
        t = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (rows, cols, vals)]
        torch.cuda.synchronize()
        A.set_values_ptr(len(vals), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), add=add)
        if keep is not None:
            keep.append(t)


def snapshot(mi, A, seed=3):
    """everything the tests compare: the three blocks, the column map and a product with a seeded vector"""
    out = {}
    for w in (0, 1, 2):
        ia, ja, a, shape = mi.parcsr_csr(A, w)
        out[f"ia{w}"], out[f"ja{w}"], out[f"a{w}"] = ia, ja, a.view(np.int64)
        out[f"shape{w}"] = np.array(shape)
    out["colmap"] = mi.parcsr_colmap(A)
    nloc = A.iupper - A.ilower + 1
    xv = np.random.default_rng(seed).standard_normal(nloc)
    x = mi.IJVector(A.ilower, A.iupper, xv)
    y = mi.IJVector(A.ilower, A.iupper, np.zeros(nloc))
    mi.call("HYPRE_ParCSRMatrixMatvec", 1.0, A.par, x.par, 0.0, y.par)
    out["matvec"] = y.get().view(np.int64)
    return out


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
    return True
