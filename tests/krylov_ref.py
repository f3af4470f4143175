"""Plain extended-precision restatements of the Krylov solvers: right-preconditioned restarted
GMRES / FlexGMRES, PCG and BiCGSTAB with HYPRE's stopping rules, written from the mathematics on dense numpy
`np.longdouble` arrays.  They are the specification the CPU oracle (tests/test_krylov_spec.py) and the device loops
(tests/test_gpu_krylov_paths.py) are compared with; nothing here is fast or clever.

Common conventions (gmres.c, flexgmres.c, pcg.c, bicgstab.c):
  * the residual-based solvers stop when the residual norm estimate is <= eps = max(atol, tol * den) with
    den = ||b|| (||r0|| when b = 0) and at least `min_iter` iterations were made, and the explicitly computed
    residual b - A x confirms it; `max_iter` ends the solve wherever it stands, with return code 256;
  * a NaN in the first norms or in an estimate ends the solve with return code 1 and without touching x again;
  * `norms` holds the initial norm and the estimate of every iteration.

GMRES keeps no Givens rotations: every step solves min ||beta e1 - H y|| on the whole Hessenberg matrix by a
Householder QR in extended precision (numpy's lstsq is double precision only: the estimate of a residual reduced by
1e-10 would keep about six digits), and every restart begins from the true residual.  GMRES, COGMRES with one or two
classical Gram-Schmidt passes and FlexGMRES build the same Krylov space; FlexGMRES only differs in x += sum y_j z_j
with the stored z_j = M v_j, which is the same vector for a fixed linear M.

Every solver returns dict(x, iters, norms, converged, code, rel_res, eps, tested): `eps` is the threshold in the units
of `norms`, `tested` every value that was compared with it while `min_iter` allowed a stop -- a case whose `tested`
values all stay clear of eps cannot change its iteration count under rounding errors."""
import numpy as np

LD = np.longdouble


def _ld(a):
    return np.asarray(a, dtype=LD)


def _norm(v):
    return np.sqrt(v @ v)


def _isnan(v):
    return bool(v != v)


def lstsq_residual(H, beta):
    """min_y ||beta e1 - H y||_2 for a full-column-rank (k+1) x k matrix: (y, the minimum), by Householder QR."""
    R = np.array(H, dtype=LD)
    m, k = R.shape
    g = np.zeros(m, dtype=LD)
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
    y = np.zeros(k, dtype=LD)
    for j in range(k - 1, -1, -1):
        y[j] = (g[j] - R[j, j + 1:k] @ y[j + 1:]) / R[j, j]
    return y, _norm(g[k:])


def dense_precond(B):
    """the preconditioner r -> B r of a tabulated linear map"""
    B = _ld(B)
    return lambda r: B @ r


def per_component(M, ncomp):
    """the preconditioner of kron(I_ncomp, A): M on every component of a component-major multivector"""
    if M is None or ncomp == 1:
        return M
    return lambda r: np.concatenate([M(c) for c in np.split(r, ncomp)])


def block_operator(A, ncomp):
    """kron(I_ncomp, A), dense"""
    return np.kron(np.eye(ncomp), np.asarray(A, dtype=np.float64)) if ncomp > 1 else A


def _result(x, iters, norms, converged, code, rel_res, eps=np.nan, tested=()):
    return dict(x=np.asarray(x, dtype=np.float64), iters=iters, norms=np.asarray(norms, dtype=np.float64),
                converged=converged, code=code, rel_res=float(rel_res), eps=float(eps),
                tested=np.asarray(tested, dtype=np.float64))


def gmres(A, b, x0=None, M=None, tol=1e-6, atol=0.0, max_iter=100, min_iter=0, kdim=50, flexible=False):
    A, b = _ld(A), _ld(b)
    x = np.zeros_like(b) if x0 is None else _ld(x0).copy()
    apply_m = (lambda v: v) if M is None else M
    r = b - A @ x
    b_norm, r_norm = _norm(b), _norm(r)
    den = b_norm if b_norm > 0 else r_norm
    eps = max(LD(atol), LD(tol) * den)
    norms, iters, converged, tested = [r_norm], 0, False, []
    rel = lambda rn: rn / b_norm if b_norm > 0 else rn  # noqa: E731
    if _isnan(b_norm) or _isnan(r_norm):
        return _result(x, 0, norms, False, 1, rel(r_norm))
    while True:
        if iters >= min_iter:
            tested.append(r_norm)
        if r_norm == 0 or (r_norm <= eps and iters >= min_iter):  # r is the true residual here
            converged = True
            break
        if iters >= max_iter:
            break
        beta = r_norm
        V, Z = [r / beta], []
        H = np.zeros((kdim + 1, kdim), dtype=LD)
        y, est = None, r_norm
        for j in range(kdim):
            if iters >= max_iter:
                break
            Z.append(apply_m(V[j]))
            w = A @ Z[j]
            for _ in range(2):  # Gram-Schmidt, twice: orthogonal to working precision
                for i in range(j + 1):
                    h = V[i] @ w
                    H[i, j] += h
                    w = w - h * V[i]
            H[j + 1, j] = _norm(w)
            iters += 1
            y, est = lstsq_residual(H[:j + 2, :j + 1], beta)
            norms.append(est)
            if _isnan(est):
                return _result(x, iters, norms, False, 1, rel(est))
            if iters >= min_iter:
                tested.append(est)
            if (est <= eps and iters >= min_iter) or H[j + 1, j] == 0:
                break
            V.append(w / H[j + 1, j])
        k = len(y)
        if flexible:
            x = x + sum(y[i] * Z[i] for i in range(k))
        else:
            x = x + apply_m(sum(y[i] * V[i] for i in range(k)))
        r = b - A @ x
        if est <= eps and iters >= min_iter:
            r_norm = _norm(r)  # the estimate is confirmed (or not) by the true residual at the top of the loop
        elif iters >= max_iter:
            r_norm = est       # gmres.c reports the estimate when the iterations run out
            break
        else:
            r_norm = _norm(r)
    code = 0 if converged or not (iters >= max_iter and r_norm > eps) else 256
    return _result(x, iters, norms, converged, code, rel(r_norm), eps, tested)


def fgmres(A, b, **kw):
    return gmres(A, b, flexible=True, **kw)


def pcg(A, b, x0=None, M=None, tol=1e-6, atol=0.0, max_iter=100, min_iter=0, two_norm=0):
    """pcg.c with its default options: the measure is <M r, r> / <M b, b> (two_norm 0) or <r, r> / <b, b>
    (two_norm 1) against max(tol^2, atol^2 / <M b, b>); no recomputation of the residual.  A right-hand side with
    a non-positive <M b, b> is answered by x = 0.  norms[i] is the square root of the measure."""
    A, b = _ld(A), _ld(b)
    x = np.zeros_like(b) if x0 is None else _ld(x0).copy()
    apply_m = (lambda v: v) if M is None else M
    bi = b @ b if two_norm else apply_m(b) @ b
    if not bi > 0:
        if _isnan(bi):
            return _result(x, 0, [], False, 1, np.nan)
        return _result(np.zeros_like(b), 0, [], True, 0, 0.0)
    eps = LD(tol) ** 2
    if atol > 0:
        eps = max(eps, LD(atol) ** 2 / bi)
    r = b - A @ x
    p = apply_m(r)
    gamma = r @ p
    measure = r @ r if two_norm else gamma
    norms = [np.sqrt(abs(measure) / bi)]
    iters, converged, tested = 0, False, []
    if _isnan(measure):
        return _result(x, 0, norms, False, 1, norms[-1])
    while iters < max_iter:
        iters += 1
        s = A @ p
        sp = s @ p
        if sp == 0:  # no direction left (an exact guess): pcg.c leaves the loop inside its first iteration
            break
        alpha = gamma / sp
        x = x + alpha * p
        r = r - alpha * s
        z = apply_m(r)
        gamma_new = r @ z
        measure = r @ r if two_norm else gamma_new
        norms.append(np.sqrt(abs(measure) / bi))
        if _isnan(measure):
            return _result(x, iters, norms, False, 1, norms[-1])
        if iters >= min_iter:
            tested.append(norms[-1])
        if measure / bi < eps and iters >= min_iter:
            converged = True
            break
        p = z + (gamma_new / gamma) * p
        gamma = gamma_new
    code = 256 if (not converged and iters >= max_iter) else 0
    return _result(x, iters, norms, converged, code, np.sqrt(abs(measure) / bi), np.sqrt(eps), tested)


def bicgstab(A, b, x0=None, M=None, tol=1e-6, atol=0.0, max_iter=100, min_iter=0):
    """bicgstab.c: right-preconditioned BiCGSTAB with the shadow residual r0; the convergence test is made after
    the half step and after the full step, each confirmed by the true residual; the breakdowns <r0, A M p> = 0,
    rho = 0 and omega = 0 leave the loop without an error."""
    A, b = _ld(A), _ld(b)
    x = np.zeros_like(b) if x0 is None else _ld(x0).copy()
    apply_m = (lambda v: v) if M is None else M
    tiny = LD(1e-128)
    r = b - A @ x
    rs, p = r.copy(), r.copy()
    b_norm = _norm(b)
    rho = rs @ r
    r_norm = np.sqrt(rho)
    den = b_norm if b_norm > 0 else r_norm
    eps = max(LD(atol), LD(tol) * den)
    norms, iters, tested = [r_norm], 0, []
    converged = bool(r_norm == 0)
    rel = lambda rn: rn / b_norm if b_norm > 0 else rn  # noqa: E731
    if _isnan(b_norm) or _isnan(r_norm):
        return _result(x, 0, norms, False, 1, rel(r_norm))

    def confirmed(xc):
        tn = _norm(b - A @ xc)
        tested.append(tn)
        return tn if tn <= eps else None

    while not converged and iters < max_iter:
        iters += 1
        v = apply_m(p)
        q = A @ v
        d = rs @ q
        if abs(d) < tiny:
            break
        alpha = rho / d
        x = x + alpha * v
        r = r - alpha * q
        r_norm = _norm(r)
        if iters >= min_iter:
            tested.append(r_norm)
        if r_norm <= eps and iters >= min_iter:
            tn = confirmed(x)
            if tn is not None:
                r_norm = tn
                norms.append(r_norm)
                converged = True
                break
        v = apply_m(r)
        t = A @ v
        tt = t @ t
        omega = (r @ t) / tt if tt != 0 else LD(0)
        x = x + omega * v
        r = r - omega * t
        r_norm = _norm(r)
        norms.append(r_norm)
        if _isnan(r_norm):
            return _result(x, iters, norms, False, 1, rel(r_norm))
        if iters >= min_iter:
            tested.append(r_norm)
        if r_norm <= eps and iters >= min_iter:
            tn = confirmed(x)
            if tn is not None:
                r_norm = tn
                converged = True
                break
        if abs(rho) < tiny:
            break
        rho_new = rs @ r
        p = p - omega * q
        if abs(omega) < tiny:
            break
        p = r + (rho_new / rho) * (alpha / omega) * p
        rho = rho_new
    code = 256 if (not converged and iters >= max_iter) else 0
    return _result(x, iters, norms, converged, code, rel(r_norm), eps, tested)
