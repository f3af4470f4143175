"""Independent plain-Python statements of the interpolation formulas of the default hierarchy, general in sign:
extended+i (De Sterck / Falgout / Nolting / Yang 2008, "Distance-two interpolation for parallel algebraic multigrid")
and classical modified interpolation (Ruge / Stueben with HYPRE's modification).  Written for the tests, sharing no code
with the oracle or the library; the strength graph comes from agg2s_ref.strength_rows, which states the mirrored rule
for rows with a negative diagonal and the max_row_sum rule.

Two rules that the published formulas leave open are stated here the way this project specifies them:
  * a strong F neighbour k whose distribution sum is zero is lumped into the diagonal;
  * a strong neighbour k that is a SPECIAL F point -- an F point whose own row kept no strong connection -- does not
    belong to F_i: it distributes nothing and its coupling a_ik goes into the diagonal like a weak one."""
import numpy as np
import scipy.sparse as sp

from tests.agg2s_ref import strength_rows


def strength_pattern(A, theta=0.57, max_row_sum=0.9):
    """0/1 CSR pattern of the strength graph (diagonal excluded): row i holds the points i depends on strongly."""
    A = sp.csr_matrix(A)
    strong = strength_rows(A, theta, max_row_sum)
    indptr = np.concatenate([[0], np.cumsum([len(s) for s in strong])])
    indices = np.concatenate([np.asarray(s, dtype=np.int64) for s in strong] + [np.zeros(0, dtype=np.int64)])
    return sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=A.shape)


def _rows_and_strong(A, S):
    A, S = sp.csr_matrix(A), sp.csr_matrix(S)
    n = A.shape[0]
    rows = [dict(zip(A.indices[A.indptr[i]:A.indptr[i + 1]], A.data[A.indptr[i]:A.indptr[i + 1]])) for i in range(n)]
    strong = [set(S.indices[S.indptr[i]:S.indptr[i + 1]]) for i in range(n)]
    return rows, strong


def special_f_points(S, cf):
    """F points whose own strong row is empty."""
    S = sp.csr_matrix(S)
    return (np.asarray(cf) != 1) & (np.diff(S.indptr) == 0)


def extended_i_reference(A, S, cf, census=None, only_rows=None):
    """P (no truncation) by the extended+i formula: for an F point i with strong C neighbours C_i, strong F neighbours
    F_i (special F points excepted) and Chat_i = C_i U (U_{k in F_i} C_k):
        w_ij = -(1 / att_i) (a_ij + sum_{k in F_i} a_ik abar_kj / d_ik),  j in Chat_i,
        att_i = a_ii + sum_{n weak or special-F neighbour of i, n not in Chat_i} a_in + sum_{k in F_i} a_ik abar_ki / d_ik,
        d_ik = sum_{l in Chat_i U {i}} abar_kl,   abar_kl = a_kl if its sign differs from a_kk's, else 0;
    a k in F_i with d_ik = 0 adds a_ik to att_i instead.  census (a dict) counts the special-F and zero-sum events.
    only_rows: the F rows to compute (the others stay empty, and out of the census); default all."""
    rows, strong = _rows_and_strong(A, S)
    n = len(rows)
    cf = np.asarray(cf)
    special = special_f_points(S, cf)
    cidx = -np.ones(n, dtype=int)
    cidx[cf == 1] = np.arange(int((cf == 1).sum()))
    P = sp.lil_matrix((n, int((cf == 1).sum())))
    count = dict(special_f=0, zero_sum=0)

    def abar(k, l):
        v = rows[k].get(l, 0.0)
        return v if v * rows[k][k] < 0 else 0.0

    for i in range(n):
        if cf[i] == 1:
            P[i, cidx[i]] = 1.0
            continue
        if only_rows is not None and i not in only_rows:
            continue
        Ci = [j for j in strong[i] if cf[j] == 1]
        Fi = [k for k in strong[i] if cf[k] != 1 and not special[k]]
        lumped = [k for k in strong[i] if cf[k] != 1 and special[k]]
        chat = set(Ci)
        for k in Fi:
            chat |= {j for j in strong[k] if cf[j] == 1}
        if not chat:
            continue
        count["special_f"] += len(lumped)
        att = rows[i][i]
        for nb, v in rows[i].items():
            if nb != i and (nb not in strong[i] or nb in lumped) and nb not in chat:
                att += v
        w = {j: rows[i].get(j, 0.0) for j in chat}
        for k in Fi:
            d = sum(abar(k, l) for l in chat | {i})
            if d == 0.0:
                count["zero_sum"] += 1
                att += rows[i][k]
                continue
            f = rows[i][k] / d
            for j in chat:
                w[j] += f * abar(k, j)
            att += f * abar(k, i)
        for j, v in w.items():
            P[i, cidx[j]] = -v / att
    if census is not None:
        census.update(count)
    return P.tocsr()


def classical_modified_reference(A, S, cf, census=None, only_rows=None):
    """P (no truncation) by classical modified interpolation: for an F point i with strong C neighbours C_i,
        w_ij = -(a_ij + sum_{k in F_i} a_ik abar_kj / sum_{m in C_i} abar_km) / (a_ii + sum_{weak or special-F n} a_in),
    abar as above; a strong F neighbour without a common C point (zero distribution sum) is lumped into the diagonal.
    census, only_rows: as in extended_i_reference."""
    rows, strong = _rows_and_strong(A, S)
    n = len(rows)
    cf = np.asarray(cf)
    special = special_f_points(S, cf)
    cidx = -np.ones(n, dtype=int)
    cidx[cf == 1] = np.arange(int((cf == 1).sum()))
    P = sp.lil_matrix((n, int((cf == 1).sum())))
    count = dict(special_f=0, zero_sum=0)
    for i in range(n):
        if cf[i] == 1:
            P[i, cidx[i]] = 1.0
            continue
        if only_rows is not None and i not in only_rows:
            continue
        Ci = [j for j in strong[i] if cf[j] == 1]
        if not Ci:
            continue
        diag = rows[i][i] + sum(v for nb, v in rows[i].items() if nb != i and nb not in strong[i])
        w = {j: rows[i][j] for j in Ci}
        for k in strong[i]:
            if cf[k] == 1:
                continue
            if special[k]:
                count["special_f"] += 1
                diag += rows[i][k]
                continue
            d = sum(rows[k].get(m, 0.0) for m in Ci if rows[k].get(m, 0.0) * rows[k][k] < 0)
            if d == 0.0:
                count["zero_sum"] += 1
                diag += rows[i][k]
                continue
            for j in Ci:
                v = rows[k].get(j, 0.0)
                if v * rows[k][k] < 0:
                    w[j] += rows[i][k] * v / d
        for j, v in w.items():
            P[i, cidx[j]] = -v / diag
    if census is not None:
        census.update(count)
    return P.tocsr()
