"""numpy / scipy restatement of the Chebyshev relaxation (relax type 16; DESIGN.md section 3, "Chebyshev relaxation"):
the eigenvalue bounds of D^-1 A (Gershgorin, or CG-Lanczos on D^-1/2 A D^-1/2 from the Park-Miller vector), the interval
and the step coefficients, one sweep by the three-term recurrence, and -- independent of the recurrence -- the same
sweep through the Chebyshev residual polynomial 1 - l p(l) = T_m((theta - l) / delta) / T_m(theta / delta), applied in
longdouble to a small dense D^-1 A."""
import numpy as np
import scipy.sparse as sp
from numpy.polynomial import chebyshev as npcheb
from numpy.polynomial import polynomial as nppoly

from tests.fsai_ref import park_miller


def gershgorin(A):
    """(lambda_min, lambda_max) = (0, max_i sum_j |a_ij| / a_ii)."""
    A = sp.csr_matrix(A)
    d = A.diagonal()
    return 0.0, float((abs(A).sum(axis=1).A1 / d).max())


def cg_lanczos(A, steps, gid0=0, dot=None, dtype=np.float64, matvec=None):
    """(lambda_min, lambda_max, steps made) of D^-1/2 A D^-1/2 from `steps` CG steps with x0 = 0 and the Park-Miller
    right-hand side; the operations in the library's order.  dot / matvec: all-reduced inner product and the product
    with the GLOBAL operator when A is one rank's diag block; dtype longdouble: the same routine in extended precision."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    dot = dot or (lambda u, v: u @ v)
    d = A.diagonal().astype(dtype)
    dis = dtype(1.0) / np.sqrt(d)
    if matvec is None:
        Ad = sp.csr_matrix((A.data.astype(dtype), A.indices, A.indptr), shape=A.shape) if dtype is np.float64 else None

        def matvec(t):
            if Ad is not None:
                return Ad @ t
            out = np.zeros(n, dtype=dtype)
            np.add.at(out, np.repeat(np.arange(n), np.diff(A.indptr)), A.data.astype(dtype) * t[A.indices])
            return out
    r = park_miller(range(gid0, gid0 + n)).astype(dtype)
    p = r.copy()
    rr = dot(r, r)
    alpha, beta = [], []
    for _ in range(steps):
        if not rr > 0:
            break
        w = matvec(p * dis) * dis
        pBp = dot(p, w)
        if not pBp > 0:
            break
        al = rr / pBp
        r = r - al * w
        rr_new = dot(r, r)
        be = rr_new / rr
        alpha.append(al)
        beta.append(be)
        rr = rr_new
        p = be * p + r
    m = len(alpha)
    assert m > 0, "the estimate made no step"
    T = np.zeros((m, m), dtype=np.float64)
    for j in range(m):
        T[j, j] = float(1 / alpha[j] + (beta[j - 1] / alpha[j - 1] if j else 0))
        if j + 1 < m:
            T[j, j + 1] = T[j + 1, j] = float(np.sqrt(beta[j]) / alpha[j])
    ev = np.linalg.eigvalsh(T)
    return float(ev[0]), float(ev[-1]), m


def bounds(eig_min, eig_max, eig_est, fraction=0.3):
    """dict(eig_min, eig_max, lower, upper, theta, delta)."""
    upper = 1.1 * eig_max if eig_est > 0 else eig_max
    lower = eig_min + fraction * (upper - eig_min)
    return dict(eig_min=eig_min, eig_max=eig_max, lower=lower, upper=upper, theta=(upper + lower) / 2.0,
                delta=(upper - lower) / 2.0)


def level_bounds(A, eig_est=10, fraction=0.3, **kw):
    if eig_est == 0:
        lo, hi = gershgorin(A)
    else:
        lo, hi, _ = cg_lanczos(A, eig_est, **kw)
    return bounds(lo, hi, eig_est, fraction)


def coefficients(theta, delta, order):
    """[(a_k, b_k)] of the steps of one sweep."""
    sigma = theta / delta
    rho = 1.0 / sigma
    out = [(0.0, 1.0 / theta)]
    for _ in range(1, order):
        rho_new = 1.0 / (2.0 * sigma - rho)
        out.append((rho_new * rho, 2.0 * rho_new / delta))
        rho = rho_new
    return out


def sweep(A, f, u, theta, delta, order, diag=None):
    """One sweep by the recurrence; u None = zero guess.  diag: the divisor when it is not A's own diagonal."""
    A = sp.csr_matrix(A)
    dg = A.diagonal() if diag is None else diag
    u = np.zeros_like(f) if u is None else u.copy()
    d = np.zeros_like(f)
    for a, b in coefficients(theta, delta, order):
        res = f - A @ u
        d = a * d + b * (res / dg)
        u = u + d
    return u


def residual_polynomial(theta, delta, order):
    """power-basis coefficients (longdouble, ascending) of q(l) = T_m((theta - l) / delta) / T_m(theta / delta)."""
    # T_m as a power series in t, then t = (theta - l) / delta
    tm = npcheb.cheb2poly([0] * order + [1]).astype(np.longdouble)
    lin = np.array([theta / delta, -1.0 / delta], dtype=np.longdouble)
    q = np.zeros(1, dtype=np.longdouble)
    pw = np.ones(1, dtype=np.longdouble)
    for c in tm:
        q = nppoly.polyadd(q, c * pw)
        pw = nppoly.polymul(pw, lin)
    return q / nppoly.polyval(np.longdouble(0.0), q)


def sweep_closed_form(A, f, u, theta, delta, order):
    """The same sweep without the recurrence: u + p(D^-1 A) D^-1 (f - A u) with p(l) = (1 - q(l)) / l, in longdouble on
    the dense operator."""
    M = np.asarray(sp.csr_matrix(A).todense()).astype(np.longdouble)
    dg = np.diag(M).copy()
    q = residual_polynomial(theta, delta, order)
    assert abs(q[0] - 1) < 1e-15
    p = -q[1:]  # (1 - q(l)) / l
    K = M / dg[:, None]
    u = np.zeros(len(f), dtype=np.longdouble) if u is None else u.astype(np.longdouble)
    z = (f.astype(np.longdouble) - M @ u) / dg
    acc = np.zeros_like(z)
    for c in p[::-1]:  # Horner in K
        acc = K @ acc + c * z
    return u + acc
