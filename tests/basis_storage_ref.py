"""Restarted right-preconditioned GMRES / FlexGMRES with the Krylov basis stored in fp32 ("Krylov
basis storage"), restated from the specification on dense numpy arrays.  It imports nothing from the library and nothing
from the other restatements; tests/test_basis_storage_spec.py compares it with tests/krylov_ref.gmres where the two must
agree, and tests/test_gpu_basis_storage.py compares the device loops with it.

The specification, with rd(v) = (double)(float)v elementwise, round to nearest even:
  * p_0 = rd(r / ||r||) and p_i = rd(w / sqrt(||w||^2)): the product first, then the rounding;
  * whatever reads a basis vector reads the rounded values: the preconditioner, through it the mat-vec, every
    Gram-Schmidt pass, and the update x += M sum_j y_j p_j;
  * h_{i+1,i} = ||w|| of the unrounded w; every sum, the Hessenberg matrix, the directions z_j = M p_j and x keep the
    working precision;
  * every restart begins from the true residual b - A x;
  * the stopping rules are gmres.c's: the estimate <= eps = max(atol, tol * den), den = ||b|| (||r_0|| when b = 0), has
    to be confirmed by the true residual, else the solve goes on from that residual ("false convergence").

`rounding=False` leaves the basis unrounded: plain GMRES.  `arith="float64"` runs the same steps in double precision
with ONE modified Gram-Schmidt pass per step, as the device loop does; the default is np.longdouble with two passes
(orthogonal to working precision against the stored vectors).  The difference between the two is the rounding error a
double-precision loop may legitimately show: the bar of the device test is measured from it.

Returns dict(x, iters, norms, converged, code, rel_res, eps, tested, false_convergences); `tested` holds every value
that was compared with eps."""
import numpy as np


def rd(v):
    """(double)(float)v in the array's own type"""
    return np.asarray(v).astype(np.float32).astype(np.asarray(v).dtype)


def _norm(v):
    return np.sqrt(v @ v)


def _least_squares(H, beta, dt):
    """min_y ||beta e1 - H y|| for a (k+1) x k Hessenberg matrix of full column rank by Householder QR: (y, the minimum)"""
    R = np.array(H, dtype=dt)
    m, k = R.shape
    g = np.zeros(m, dtype=dt)
    g[0] = beta
    for j in range(k):
        v = R[j:, j].copy()
        nv = _norm(v)
        if nv == 0:
            continue
        v[0] += nv if v[0] >= 0 else -nv
        vv = v @ v
        if vv == 0:
            continue
        R[j:, j:] -= np.outer(v, (2 / vv) * (v @ R[j:, j:]))
        g[j:] -= v * ((2 / vv) * (v @ g[j:]))
    y = np.zeros(k, dtype=dt)
    for j in range(k - 1, -1, -1):
        y[j] = (g[j] - R[j, j + 1:k] @ y[j + 1:]) / R[j, j]
    return y, _norm(g[k:])


def gmres(A, b, x0=None, M=None, tol=1e-6, atol=0.0, max_iter=100, min_iter=0, kdim=50, flexible=False, rounding=True,
          arith="longdouble"):
    """M: a callable r -> M r working on arrays of the arithmetic's type (None: no preconditioner)"""
    assert arith in ("longdouble", "float64")
    dt = np.longdouble if arith == "longdouble" else np.float64
    passes = 2 if arith == "longdouble" else 1
    stored = rd if rounding else (lambda v: v)
    A, b = np.asarray(A, dtype=dt), np.asarray(b, dtype=dt)
    x = np.zeros_like(b) if x0 is None else np.asarray(x0, dtype=dt).copy()
    apply_m = (lambda v: v) if M is None else M
    r = b - A @ x
    b_norm, r_norm = _norm(b), _norm(r)
    den = b_norm if b_norm > 0 else r_norm
    eps = max(dt(atol), dt(tol) * den)
    norms, iters, converged, tested, false_conv = [r_norm], 0, False, [], 0
    est = r_norm
    while True:
        # r is the true residual here
        if iters >= min_iter:
            tested.append(r_norm)
        if r_norm == 0 or (r_norm <= eps and iters >= min_iter):
            converged = True
            break
        if iters >= max_iter:
            break
        beta = r_norm
        V, Z = [stored(r * (1 / beta))], []
        H = np.zeros((kdim + 1, kdim), dtype=dt)
        y = None
        for j in range(kdim):
            if iters >= max_iter:
                break
            Z.append(apply_m(V[j]))
            w = A @ Z[j]
            for _ in range(passes):
                for i in range(j + 1):
                    h = V[i] @ w
                    H[i, j] += h
                    w = w - h * V[i]
            H[j + 1, j] = np.sqrt(w @ w)
            iters += 1
            y, est = _least_squares(H[:j + 2, :j + 1], beta, dt)
            norms.append(est)
            if iters >= min_iter:
                tested.append(est)
            if (est <= eps and iters >= min_iter) or H[j + 1, j] == 0:
                break
            V.append(stored(w * (1 / H[j + 1, j])))
        k = len(y)
        if flexible:
            x = x + sum(y[i] * Z[i] for i in range(k))
        else:
            x = x + apply_m(sum(y[i] * V[i] for i in range(k)))
        r = b - A @ x
        true_norm = _norm(r)
        if est <= eps and iters >= min_iter:
            if true_norm > eps:
                false_conv += 1
            r_norm = true_norm
        elif iters >= max_iter:
            r_norm = est  # gmres.c reports the estimate when the iterations run out
            break
        else:
            r_norm = true_norm
    code = 0 if converged or not (iters >= max_iter and r_norm > eps) else 256
    rel = r_norm / b_norm if b_norm > 0 else r_norm
    return dict(x=np.asarray(x, dtype=np.float64), iters=iters, norms=np.asarray(norms, dtype=np.float64),
                converged=converged, code=code, rel_res=float(rel), eps=float(eps),
                tested=np.asarray(tested, dtype=np.float64), false_convergences=false_conv)


def dense_precond(B, arith="longdouble"):
    """the preconditioner r -> B r of a tabulated linear map"""
    B = np.asarray(B, dtype=np.longdouble if arith == "longdouble" else np.float64)
    return lambda r: B @ r


def per_component(M, ncomp):
    """M on every component of a component-major multivector: the preconditioner of kron(I_ncomp, A)"""
    if M is None or ncomp == 1:
        return M
    return lambda r: np.concatenate([M(c) for c in np.split(r, ncomp)])


def laplace_7pt(n):
    """the 7-point Laplacian on an n^3 grid (diagonal 6, off-diagonals -1), dense float64"""
    T = 2 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
    eye = np.eye(n)
    return np.kron(np.kron(T, eye), eye) + np.kron(np.kron(eye, T), eye) + np.kron(np.kron(eye, eye), T)


def sgs_matrix(A):
    """symmetric Gauss-Seidel as a dense map: (D + U)^-1 D (D + L)^-1"""
    A = np.asarray(A, dtype=np.float64)
    D = np.diag(np.diag(A))
    return np.linalg.solve(np.triu(A), D @ np.linalg.inv(np.tril(A)))
