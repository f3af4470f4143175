"""numpy restatement of the distance-1 approximate ideal restriction (HYPRE_BoomerAMGSetRestriction 1) and of the
one-point interpolation (interp_type 100) from their definitions in DESIGN.md section 3 -- independent of the
library's routines: the local systems go to np.linalg.solve (float64) or to a plain elimination in np.longdouble,
not to the elimination order the library documents.  Also the two-grid cycle (C/F Jacobi, exact coarse solve) in
dense algebra."""
import numpy as np
import scipy.sparse as sp


def neighbourhoods(A, cf, theta_r):
    """N_i of every C point i (ascending), in the order of the C points: the F columns j != i of row i with
    |a_ij| >= theta_r * max_{k != i} |a_ik|; empty when that maximum is 0"""
    A = sp.csr_matrix(A)
    out = []
    for i in np.flatnonzero(np.asarray(cf) == 1):
        cols = A.indices[A.indptr[i]:A.indptr[i + 1]]
        vals = np.abs(A.data[A.indptr[i]:A.indptr[i + 1]])
        off = cols != i
        mx = vals[off].max(initial=0.0)
        if mx == 0.0:
            out.append(np.zeros(0, dtype=np.int64))
            continue
        keep = off & (vals >= theta_r * mx) & (np.asarray(cf)[cols] != 1)
        out.append(np.sort(cols[keep]).astype(np.int64))
    return out


def solve_longdouble(M, b):
    """M y = b by Gaussian elimination with partial pivoting (rows swapped) in np.longdouble"""
    M = np.array(M, dtype=np.longdouble)
    b = np.array(b, dtype=np.longdouble)
    m = len(b)
    for k in range(m):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]] = M[[p, k]]
            b[[k, p]] = b[[p, k]]
        l = M[k + 1:, k] / M[k, k]
        M[k + 1:, k:] -= np.outer(l, M[k, k:])
        b[k + 1:] -= l * b[k]
    y = np.zeros(m, dtype=np.longdouble)
    for k in range(m - 1, -1, -1):
        y[k] = (b[k] - M[k, k + 1:] @ y[k + 1:]) / M[k, k]
    return y


def air_restriction(A, cf, theta_r=0.25, phi=0.0, longdouble=False):
    """R (|C| x n, explicit zeros kept): row c(i) = (N_t, y_t) with A[N_i, N_i]^T y = -A[i, N_i]^T, less the entries with
    |y_t| < phi * max_s |y_s| (phi > 0), and (i, 1.0); columns ascending.  Values float64, or longdouble as a dense
    longdouble array beside the pattern when longdouble=True: returns (R, values) with values[k] for R.data[k]."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    cpts = np.flatnonzero(np.asarray(cf) == 1)
    indptr, indices, data = [0], [], []
    for i, N in zip(cpts, neighbourhoods(A, cf, theta_r)):
        cols, vals = [int(i)], [1.0]
        if len(N):
            sub = A[N][:, N].toarray()
            g = A[i][:, N].toarray().ravel()
            if longdouble:
                y = solve_longdouble(np.array(sub.T, dtype=np.longdouble), -np.array(g, dtype=np.longdouble))
            else:
                y = np.linalg.solve(sub.T, -g)
            keep = np.ones(len(N), dtype=bool)
            if phi > 0.0:
                keep = ~(np.abs(y) < phi * np.abs(y).max())
            cols += [int(j) for j in N[keep]]
            vals += list(y[keep])
        o = np.argsort(cols, kind="stable")
        indices += [cols[q] for q in o]
        data += [vals[q] for q in o]
        indptr.append(len(indices))
    exact = np.array(data, dtype=np.longdouble if longdouble else np.float64)
    R = sp.csr_matrix((exact.astype(np.float64), np.array(indices, dtype=np.int64), np.array(indptr)), shape=(len(cpts), n))
    return (R, exact) if longdouble else R


def one_point_interp(A, strong, cf):
    """P (n x |C|): a C point i gets (c(i), 1.0); an F point the C point j of strong[i] with the largest |a_ij|, the lowest
    column on a tie, as (c(j), 1.0); an F point without one an empty row"""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    cf = np.asarray(cf)
    c_of = np.cumsum(cf == 1) - 1
    indptr, indices = [0], []
    for i in range(n):
        if cf[i] == 1:
            indices.append(c_of[i])
        else:
            cand = sorted(int(j) for j in strong[i] if cf[j] == 1)
            if cand:
                mags = [abs(A[i, j]) for j in cand]
                indices.append(c_of[cand[int(np.argmax(mags))]])  # argmax: the first of equal maxima
        indptr.append(len(indices))
    return sp.csr_matrix((np.ones(len(indices)), np.array(indices, dtype=np.int64), np.array(indptr)), shape=(n, int((cf == 1).sum())))


def two_grid_cycle(A, P, R, Ac, cf, u, f, dtype=np.float64):
    """One cycle of the two-level method as amg_solve.cpp states it for relax_type 0, relax_order 1, one sweep each way
    and an exact coarsest solve: Jacobi on the C points, then on the F points; u += P (R A P)^-1 R (f - A u); Jacobi on
    the F points, then on the C points.  Dense arrays of `dtype`; Ac = R A P."""
    d = np.diag(A)
    c, fp = cf == 1, cf != 1
    for pts in (c, fp):
        r = f - A @ u
        u = u.copy()
        u[pts] += r[pts] / d[pts]
    r = f - A @ u
    if dtype == np.float64:
        e = np.linalg.solve(Ac, R @ r)
    else:
        e = solve_longdouble(Ac, R @ r)
    u = u + P @ e
    for pts in (fp, c):
        r = f - A @ u
        u = u.copy()
        u[pts] += r[pts] / d[pts]
    return u


def residual_history(A, P, R, cf, f, cycles, dtype=np.float64):
    """||f - A u_k|| / ||f|| for k = 0 ... cycles of the stationary two-grid iteration from u_0 = 0"""
    A, P, R = (np.array(sp.csr_matrix(M).toarray(), dtype=dtype) for M in (A, P, R))
    f = np.array(f, dtype=dtype)
    u = np.zeros_like(f)
    cf = np.asarray(cf)
    Ac = R @ A @ P
    out = [1.0]
    for _ in range(cycles):
        u = two_grid_cycle(A, P, R, Ac, cf, u, f, dtype)
        out.append(float(np.sqrt(((f - A @ u) ** 2).sum()) / np.sqrt((f ** 2).sum())))
    return np.array(out)


def two_grid_factor(A, P, R, cf, cycles=12, seed=7):
    """the stationary residual reduction per cycle: (||r_cycles|| / ||r_0||)^(1 / cycles) for a seeded random f"""
    f = np.random.default_rng(seed).standard_normal(A.shape[0])
    h = residual_history(A, P, R, cf, f, cycles)
    return float(h[-1] ** (1.0 / cycles))
