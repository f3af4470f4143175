"""Inputs and helpers of the IJ value-update tests (test_ij_update_spec.py on the CPU, test_gpu_ij_update.py and its
workers on the GPU).  A round is a list of operations in call order: a batch (rows, cols, vals, add) as in
tests/ij_cases.py, or ("const", value) for HYPRE_IJMatrixSetConstantValues.  The oracle of a sequence of rounds without
constants is ONE fresh assembly of all batches concatenated (cases.fold); a constant c is, for the oracle, a Set batch
that holds every pair of the pattern once with the value c."""
import numpy as np

from tests import ij_cases as cases

BIG = cases.BIG


def pattern_of(batches):
    """the distinct (row, column) pairs of the batches, sorted"""
    pairs = set()
    for rows, cols, _, _ in batches:
        pairs.update(zip(rows.tolist(), cols.tolist()))
    return sorted(pairs)


def batch(entries, add):
    a = np.array(entries, dtype=np.float64).reshape(-1, 3)
    return (a[:, 0].astype(np.int64), a[:, 1].astype(np.int64), np.ascontiguousarray(a[:, 2]), add)


def const_as_batch(pairs, value):
    a = np.array(pairs, dtype=np.int64).reshape(-1, 2)
    return (a[:, 0].copy(), a[:, 1].copy(), np.full(len(a), float(value)), False)


def oracle_batches(rounds, pairs):
    """the rounds as one list of batches for a fresh assembly"""
    out = []
    for ops in rounds:
        for op in ops:
            out.append(const_as_batch(pairs, op[1]) if isinstance(op[0], str) else op)
    return out


def apply_round(mi, A, ops, device=False, host_only=False, keep=None):
    for op in ops:
        if isinstance(op[0], str):
            A.set_constant_values(op[1])
        else:
            cases.stage(mi, A, [op], device, keep)
    if host_only:
        mi.call("HYPRE_MI_IJMatrixAssembleHostOnly", A.h)
    else:
        A.assemble()


def host_snapshot(mi, A):
    """what a CPU test can compare: the two host blocks and the column map"""
    out = {}
    for w in (0, 1):
        ia, ja, a, shape = mi.parcsr_csr(A, w)
        out[f"ia{w}"], out[f"ja{w}"], out[f"a{w}"], out[f"shape{w}"] = ia, ja, a.view(np.int64), np.array(shape)
    out["colmap"] = mi.parcsr_colmap(A)
    return out


def small_rounds():
    """duplicates_small() as round 1; round 2 on a subset of its pairs: sums that depend on the association
    (1e16, 1, -1e16 added one at a time onto the stored value), a Set after Adds to one pair followed by one more Add,
    duplicates inside a batch, rows 5 and 17 not mentioned; round 3: seeded Adds and Sets on another subset."""
    n, first = cases.duplicates_small()
    pairs = pattern_of(first)
    rng = np.random.default_rng(20261018)
    free = [p for p in pairs if p[0] not in (3, 5, 9)]
    pick = [free[i] for i in rng.choice(len(free), size=40, replace=False)]
    a1 = [(3, 3, BIG), (3, 3, 1.0), (3, 3, -BIG)]            # stored 0: ((0 + 1e16) + 1) - 1e16 = 0, not 1
    a1 += [(3, 4, -BIG), (3, 4, BIG)]                        # stored 1: (1 - 1e16) + 1e16 = 0
    a1 += [(3, 5, 3.0), (3, 5, 3.0)]                         # a duplicate inside the batch
    a1 += [(r, c, float(rng.choice([BIG, 1.0, -BIG, 0.5, -2.25]))) for r, c in pick[:25] for _ in range(int(rng.integers(1, 4)))]
    s2 = [(3, 5, -7.0), (9, 9, 0.0)] + [(r, c, float(rng.choice([3.0, 1e-3, 0.0]))) for r, c in pick[15:30]]
    a3 = [(3, 5, 0.5)] + [(r, c, float(rng.choice([BIG, 1.0, -BIG]))) for r, c in pick[20:40] for _ in range(2)]
    second = []
    for ent, add in ((a1, True), (s2, False), (a3, True)):
        order = rng.permutation(len(ent))
        # entries of one pair keep their order inside a batch only where the test depends on it (row 3)
        fixed = [e for e in ent if e[0] == 3]
        rest = [ent[i] for i in order if ent[i][0] != 3]
        second.append(batch(rest[: len(rest) // 2] + fixed + rest[len(rest) // 2:], add))
    pick3 = [pairs[i] for i in rng.choice(len(pairs), size=60, replace=True)]
    third = [batch([(r, c, float(rng.choice([BIG, 1.0, -BIG, 0.5]))) for r, c in pick3[:40]], True),
             batch([(r, c, float(rng.choice([2.0, -1.0]))) for r, c in pick3[30:]], False)]
    assert 5 not in set(np.concatenate([b[0] for b in second]).tolist())
    return n, pairs, [first, second, third]
