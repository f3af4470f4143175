"""Plain-numpy restatement of the FSAI smoother / preconditioner ("FSAI"): pattern, local solves,
omega by power iteration, one smoothing step.  Shared by the CPU self-checks and the GPU parity tests."""
import numpy as np
import scipy.sparse as sp

PM_MOD = 2147483647


def park_miller(gids, seed=2747):
    """element gid of the PMIS measures' Park-Miller stream: seed * 16807^(gid+1) mod (2^31 - 1), over 2^31 - 1."""
    out = np.empty(len(gids))
    for q, g in enumerate(gids):
        out[q] = (seed * pow(16807, int(g) + 1, PM_MOD) % PM_MOD) / PM_MOD
    return out


def pattern(B, theta=0.01, k=1):
    """P_i = {j <= i : (S^k)_ij != 0}, S = the threshold-filtered graph of B with the diagonal (structural)."""
    B = sp.csr_matrix(B)
    B.sort_indices()
    n = B.shape[0]
    rows, cols = [], []
    for i in range(n):
        js = B.indices[B.indptr[i]:B.indptr[i + 1]]
        vs = np.abs(B.data[B.indptr[i]:B.indptr[i + 1]])
        off = js != i
        mx = vs[off].max() if off.any() else 0.0
        keep = (js == i) | (vs >= theta * mx)
        kj = set(js[keep].tolist()) | {i}
        rows += [i] * len(kj)
        cols += sorted(kj)
    S = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n))
    Sk = S.copy()
    for _ in range(k - 1):
        Sk = Sk @ S
    L = sp.tril(Sk).tocsr()
    L.sort_indices()
    return [L.indices[L.indptr[i]:L.indptr[i + 1]].copy() for i in range(n)]


def local_solve(M):
    """y with M^T y = e_last: Gaussian elimination with partial pivoting (largest |value|, lowest row on a tie), rows
    not moved, back substitution by columns in descending order -- the kernel's order of operations."""
    At = np.array(M, dtype=np.float64).T.copy()
    m = At.shape[0]
    rhs = np.zeros(m)
    rhs[m - 1] = 1.0
    used = np.zeros(m, dtype=bool)
    piv = np.zeros(m, dtype=np.int64)
    step = np.full(m, m)
    for k in range(m):
        cand = np.where(~used)[0]
        v = np.abs(At[cand, k])
        best = cand[np.argmax(v)]  # argmax: the first (lowest row) of equal maxima
        if not (np.abs(At[best, k]) > 0.0):
            raise np.linalg.LinAlgError("singular")
        piv[k] = best
        used[best] = True
        step[best] = k
        for r in np.where(~used)[0]:
            l = At[r, k] / At[best, k]
            At[r, k + 1:] = At[r, k + 1:] - l * At[best, k + 1:]
            rhs[r] = rhs[r] - l * rhs[best]
    y = np.zeros(m)
    for c in range(m - 1, -1, -1):
        p = piv[c]
        y[c] = rhs[p] / At[p, c]
        for r in range(m):
            if step[r] < c:
                rhs[r] = rhs[r] - At[r, c] * y[c]
    return y


def factor(B, theta=0.01, k=1, pat=None):
    """G (scipy CSR, lower triangular) of FSAI with the static pattern."""
    B = sp.csr_matrix(B)
    Bd = B.toarray() if B.shape[0] <= 4096 else None
    n = B.shape[0]
    P = pattern(B, theta, k) if pat is None else pat
    indptr, idx, val = [0], [], []
    for i in range(n):
        p = P[i]
        assert len(p) <= 64 and p[-1] == i
        M = Bd[np.ix_(p, p)] if Bd is not None else B[p][:, p].toarray()
        y = local_solve(M)
        if not (y[-1] > 0.0):
            raise ValueError(f"y_last <= 0 in row {i}")
        idx += p.tolist()
        val += (y / np.sqrt(y[-1])).tolist()
        indptr.append(len(idx))
    return sp.csr_matrix((np.array(val), np.array(idx), np.array(indptr)), shape=(n, n))


def omega(G, B, iters=5, gid0=0, dot=None):
    """1 / (Rayleigh quotient of G B G^T after `iters` power iterations from the Park-Miller vector); dot: the
    all-reduced inner product (multi-rank), default the local one."""
    dot = dot or (lambda a, b: float(a @ b))
    v = park_miller(range(gid0, gid0 + B.shape[0]))
    lam = 0.0
    for _ in range(iters):
        w = G @ (B @ (G.T @ v))
        lam = dot(v, w) / dot(v, v)
        v = w / np.sqrt(dot(w, w))
    return 1.0 / lam


def smooth(G, om, A, f, u=None):
    """one step u + omega G^T G (f - A u); u None = zero guess."""
    r = f if u is None else f - A @ u
    du = om * (G.T @ (G @ r))
    return du if u is None else u + du
