"""Reference for the steps a BoomerAMG cycle runs between two relaxation calls (tests/test_gpu_cycle_steps.py,
tests/test_cycle_steps_spec.py): residual, restriction, prolongation, collapsed map.  numpy only.

Every step is recomputed in np.longdouble (64-bit significand) from the vectors the cycle trace recorded and the level's
own operators as level_csr reports them (the stored values).  The checks are per row, against the standard a-priori
bound for a sum of k rounded products taken in any order, contracted or not (Higham, Accuracy and Stability of Numerical
Algorithms, section 3.1): with u = 2^-53 and gamma_k = k u / (1 - k u),

  residual      | r_i - (f_i - sum_j a_ij u_j) |  <=  gamma_{m_i + 2} (|f_i| + sum_j |a_ij| |u_j|)
                (+2: the subtraction, and the composite path subtracts in two stages)
  restriction   | fc_i - sum_j r_ij r_j |         <=  gamma_{m_i} sum_j |r_ij| |r_j|
  prolongation  | v_i - (u_i + sum_j p_ij e_j) |  <=  gamma_{m_i + 1} (|u_i| + sum_j |p_ij| |e_j|); a row of P without
                entries keeps the bits of u_i
  collapsed map | u_i - sum_j B_ij f_j |          <=  gamma_n sum_j |B_ij| |f_j|

m_i = the stored entries of row i.  Nothing here is measured from the code under test."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the reference needs a long double with a 64-bit significand"
U = 2.0 ** -53


def gamma(k):
    ku = np.asarray(k, dtype=LD) * LD(U)
    return ku / (LD(1) - ku)


class Csr:
    """(ia, ja, a, shape) as level_csr returns it"""

    def __init__(self, ia, ja, a, shape):
        self.ia = np.asarray(ia, dtype=np.int64)
        self.ja = np.asarray(ja, dtype=np.int64)
        self.a = np.asarray(a, dtype=np.float64)
        self.shape = tuple(int(s) for s in shape)
        assert len(self.ia) == self.shape[0] + 1 and len(self.ja) == self.ia[-1] == len(self.a)
        assert len(self.ja) == 0 or (self.ja.min() >= 0 and self.ja.max() < self.shape[1])
        self.rows = np.repeat(np.arange(self.shape[0]), np.diff(self.ia))
        self.m = np.diff(self.ia)

    def products(self, x):
        """(sum_j a_ij x_j, sum_j |a_ij| |x_j|) per row, in long double"""
        x = np.asarray(x, dtype=np.float64)
        assert x.shape == (self.shape[1],)
        prod = self.a.astype(LD) * x.astype(LD)[self.ja]
        s = np.zeros(self.shape[0], dtype=LD)
        t = np.zeros(self.shape[0], dtype=LD)
        np.add.at(s, self.rows, prod)
        np.add.at(t, self.rows, np.abs(prod))
        return s, t


class Verdict:
    """err and bound per row; ok = every row inside its bound (and every row that must keep its bits kept them)"""

    def __init__(self, err, bound, bits_ok=True):
        self.err, self.bound, self.bits_ok = err, bound, bool(bits_ok)
        self.bad = np.flatnonzero(~(err <= bound))  # a NaN is bad
        self.ok = self.bits_ok and len(self.bad) == 0
        pos = bound > 0
        self.ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0

    def __bool__(self):
        return self.ok

    def __repr__(self):
        if self.ok:
            return "ok, largest error %.3g of its bound" % self.ratio
        i = int(self.bad[0]) if len(self.bad) else -1
        return "FAILED: %d rows outside their bound, first row %d (err %.3e, bound %.3e), bits_ok %s" % (
            len(self.bad), i, float(self.err[i]) if i >= 0 else 0.0, float(self.bound[i]) if i >= 0 else 0.0, self.bits_ok)


def _vec(x, n):
    x = np.asarray(x, dtype=np.float64)
    assert x.shape == (n,), (x.shape, n)
    return x


def check_residual(A, f, u, r):
    n = A.shape[0]
    f, u, r = _vec(f, n), _vec(u, A.shape[1]), _vec(r, n)
    s, t = A.products(u)
    ref = f.astype(LD) - s
    return Verdict(np.abs(r.astype(LD) - ref), gamma(A.m + 2) * (np.abs(f).astype(LD) + t))


def check_restriction(R, r, fc):
    r, fc = _vec(r, R.shape[1]), _vec(fc, R.shape[0])
    s, t = R.products(r)
    return Verdict(np.abs(fc.astype(LD) - s), gamma(R.m) * t)


def check_prolongation(P, u, e, v):
    n = P.shape[0]
    u, e, v = _vec(u, n), _vec(e, P.shape[1]), _vec(v, n)
    s, t = P.products(e)
    ref = u.astype(LD) + s
    empty = P.m == 0
    bits_ok = np.array_equal(u[empty].view(np.int64), v[empty].view(np.int64))
    return Verdict(np.abs(v.astype(LD) - ref), gamma(P.m + 1) * (np.abs(u).astype(LD) + t), bits_ok)


def check_collapsed(B, f, u):
    B = np.asarray(B, dtype=np.float64)
    n = B.shape[0]
    assert B.shape == (n, n)
    f, u = _vec(f, n), _vec(u, n)
    prod = B.astype(LD) * f.astype(LD)[None, :]
    return Verdict(np.abs(u.astype(LD) - prod.sum(axis=1)), gamma(n) * np.abs(prod).sum(axis=1))


# ---- what a correct fp64 implementation may return: the row's terms added one by one in a given order (spec test)
def fp64_rowsums(A, x, order_rng=None, first=None, sign=1.0):
    """first_i + sign * (a_ij x_j added in a shuffled order), everything rounded to fp64 step by step"""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros(A.shape[0]) if first is None else np.array(first, dtype=np.float64)
    for i in range(A.shape[0]):
        idx = np.arange(A.ia[i], A.ia[i + 1])
        if order_rng is not None:
            order_rng.shuffle(idx)
        if first is None or sign == 1.0:
            acc = out[i]
            for q in idx:
                acc = acc + A.a[q] * x[A.ja[q]]
            out[i] = acc
        else:  # f - (sum): the sum first, one subtraction
            acc = 0.0
            for q in idx:
                acc = acc + A.a[q] * x[A.ja[q]]
            out[i] = out[i] - acc
    return out
