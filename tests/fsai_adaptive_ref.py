"""Plain-numpy restatement of FSAI with the adaptive pattern (fsai_algo_type 4; DESIGN.md section 3, "FSAI (adaptive
pattern)"): every row of G grows its own pattern from the Kaporin gradient.  The local solve is fsai_ref.local_solve
(the static path's elimination); the gradient is summed over the pattern's rows in ascending order, the row itself
last, one `acc = acc + b * y` per stored entry."""
import numpy as np
import scipy.sparse as sp

from tests import fsai_ref

STOP_TOL, STOP_NO_CANDIDATE, STOP_MAX_STEPS = "tolerance", "no_candidate", "max_steps"


class RowFailure(ValueError):
    """row: the failing row; kind: 1 singular local system (a missing diagonal included), 2 y_last <= 0."""

    def __init__(self, row, kind):
        super().__init__(f"FSAI local solve failed in row {row} (kind {kind})")
        self.row, self.kind = row, kind


def _solve(Bd, B, P, i):
    M = Bd[np.ix_(P, P)] if Bd is not None else B[P][:, P].toarray()
    try:
        y = fsai_ref.local_solve(M)
    except np.linalg.LinAlgError:
        raise RowFailure(i, 1) from None
    if not (y[-1] > 0.0):
        raise RowFailure(i, 2)
    return y


def grow_row(B, Bd, i, max_steps=3, max_step_size=5, kap_tolerance=1e-3):
    """(P, y, stop, psis, most candidates at a step) of row i: P ascending with i last, y the last local solution."""
    P = [i]
    y = _solve(Bd, B, P, i)
    psi = 1.0 / y[-1]
    psis = [psi]
    most = 0
    for _ in range(max_steps):
        phi = {}
        inP = set(P)
        for r, yr in zip(P, y):
            for k in range(B.indptr[r], B.indptr[r + 1]):
                j = int(B.indices[k])
                if j >= i:
                    break
                if j in inP:
                    continue
                phi[j] = phi.get(j, 0.0) + B.data[k] * yr
        cand = sorted((-abs(v), j) for j, v in phi.items() if abs(v) > 0.0)
        most = max(most, len(cand))
        if not cand:
            return P, y, STOP_NO_CANDIDATE, psis, most
        P = sorted(P[:-1] + [j for _, j in cand[:max_step_size]]) + [i]
        y = _solve(Bd, B, P, i)
        psi_new = 1.0 / y[-1]
        psis.append(psi_new)
        if psi - psi_new < kap_tolerance * psi:
            return P, y, STOP_TOL, psis, most
        psi = psi_new
    return P, y, STOP_MAX_STEPS, psis, most


def factor(B, max_steps=3, max_step_size=5, kap_tolerance=1e-3):
    """(G, info): G scipy CSR, lower triangular; info = dict(max_row, max_candidates, stops {reason: rows}, pattern,
    psi) -- the counts HYPRE_MI_FSAIAdaptiveOp reports.  Raises RowFailure for the first failing row."""
    B = sp.csr_matrix(B, dtype=np.float64)
    B.sort_indices()
    n = B.shape[0]
    Bd = B.toarray() if n <= 4096 else None
    indptr, idx, val = [0], [], []
    stops = {STOP_TOL: 0, STOP_NO_CANDIDATE: 0, STOP_MAX_STEPS: 0}
    pats, psi, most = [], [], 0
    for i in range(n):
        P, y, stop, ps, mc = grow_row(B, Bd, i, max_steps, max_step_size, kap_tolerance)
        stops[stop] += 1
        most = max(most, mc)
        pats.append(np.array(P))
        psi.append(ps)
        idx += P
        val += (y / np.sqrt(y[-1])).tolist()
        indptr.append(len(idx))
    G = sp.csr_matrix((np.array(val), np.array(idx, dtype=np.int64), np.array(indptr)), shape=(n, n))
    info = dict(max_row=int(np.diff(indptr).max()), max_candidates=most, stops=stops, pattern=pats, psi=psi)
    return G, info
