"""The blocked modified Gram-Schmidt step of single-rank GMRES, restated in numpy and set against
the chain (one coefficient per pass) in np.longdouble -- on a basis that is deliberately NOT orthogonal, so that the
forward substitution with the in-block Gram entries is what makes the two agree.  tests/test_gpu_mgs_block.py holds
the device kernel to the same restatement."""
import numpy as np
import pytest

LD = np.longdouble
B = 8


def forward_subst(c, gram, m, dtype=LD):
    """h_j = c_j - sum_{k<j} h_k g_jk for j < m, g_jk = gram[j, k] / sqrt(gram[j, B]) (0 where gram[j, B] <= 0):
    gram[j] is the raw row of basis vector j: <p_k, w_j> for k < j, then ||w_j||^2, with p_j = w_j / ||w_j||."""
    h = np.zeros(B, dtype=dtype)
    g = np.zeros((B, B), dtype=dtype)
    for j in range(m):
        nrm = dtype(gram[j][B])
        inv = dtype(1) / np.sqrt(nrm) if (j > 0 and nrm > 0) else dtype(0)
        hj = dtype(c[j])
        for k in range(j):
            g[j, k] = dtype(gram[j][k]) * inv
            hj = hj - h[k] * g[j, k]
        h[j] = hj
    return h, g


def one_pass(prev, nxt, last, c, gram, w, dtype=LD):
    """(sums, h, w_new) of one pass: subtract the block `prev` (rows) with the substituted coefficients in ascending
    order, then <nxt_j, w_new>, or in the last pass <prev_j, w_new> and, at [B], ||w_new||^2."""
    m_prev = len(prev)
    h, _ = forward_subst(c, gram, m_prev, dtype)
    wn = np.array(w, dtype=dtype)
    for j in range(m_prev):
        wn = wn - h[j] * np.asarray(prev[j], dtype=dtype)
    sums = np.zeros(B + 1, dtype=dtype)
    if last:
        for j in range(m_prev):
            sums[j] = (np.asarray(prev[j], dtype=dtype) * wn).sum()
        sums[B] = (wn * wn).sum()
    else:
        for j in range(len(nxt)):
            sums[j] = (np.asarray(nxt[j], dtype=dtype) * wn).sum()
    return sums, h, wn


def blocked_step(P, gram_rows, w, dtype=np.float64):
    """Arnoldi step i = len(P) in ceil(i / B) + 1 passes over aligned blocks: (h[0 .. i), w_final, ||w_final||^2,
    the raw Gram row of the new vector)."""
    i = len(P)
    nblk = (i + B - 1) // B
    h = np.zeros(i, dtype=dtype)
    wn = np.array(w, dtype=dtype)
    c = np.zeros(B + 1, dtype=dtype)
    for kb in range(nblk + 1):
        prev = P[(kb - 1) * B:min(kb * B, i)] if kb else []
        nxt = P[kb * B:min((kb + 1) * B, i)] if kb < nblk else []
        rows = gram_rows[(kb - 1) * B:(kb - 1) * B + B] if kb else np.zeros((B, B + 1))
        c, hb, wn = one_pass(prev, nxt, kb == nblk, c, rows, wn, dtype)
        if kb:
            h[(kb - 1) * B:(kb - 1) * B + len(prev)] = hb[:len(prev)]
    return h, wn, c[B], c


def chain_step(P, w):
    """h_j = <p_j, w>, w -= h_j p_j, one vector after the other, in extended precision"""
    wn = np.array(w, dtype=LD)
    h = np.zeros(len(P), dtype=LD)
    for j in range(len(P)):
        pj = np.asarray(P[j], dtype=LD)
        h[j] = (pj * wn).sum()
        wn = wn - h[j] * pj
    return h, wn


def skewed_basis(rng, m, n, eps=0.05):
    """m unit vectors whose Gram matrix has off-diagonal entries up to about eps, and their raw Gram rows for aligned
    blocks of B, stated through unscaled vectors w_j = s_j p_j with s_j far from 1"""
    Q, _ = np.linalg.qr(rng.standard_normal((n, m)))
    Q = Q.T
    P = np.zeros((m, n))
    for j in range(m):
        v = Q[j].copy()
        for k in range(j):
            v += rng.uniform(-eps, eps) * Q[k]
        P[j] = v / np.linalg.norm(v)
    s = rng.uniform(0.01, 100.0, m)
    rows = np.zeros((m, B + 1))
    for j in range(m):
        for k in range(j % B):
            rows[j, k] = float((P[j - j % B + k].astype(LD) * (s[j] * P[j]).astype(LD)).sum())
        rows[j, B] = float(((s[j] * P[j]).astype(LD) ** 2).sum())
    return P, rows


def step_bounds(P, rows, w):
    """Bounds for h and w of the blocked step in double precision against the chain in exact arithmetic: an inner
    product is good to 1e-13 * sum|terms| (the project's bound for its reductions), its terms p_j[e] * w[e] with w any
    of the intermediate vectors, all within |w_0| + sum_k |h_k| |p_k|; the substitution passes an error of h_k on to
    h_j times |g_jk|, which the product of (1 + |g_jk|) over the block's pairs covers."""
    i = len(P)
    h_ref, _ = chain_step(P, w)
    absw = np.abs(np.asarray(w, dtype=LD)) + (np.abs(h_ref)[:, None] * np.abs(P.astype(LD))).sum(axis=0)
    tol_h = np.zeros(i)
    for j0 in range(0, i, B):
        m = min(B, i - j0)
        _, g = forward_subst(np.zeros(B), rows[j0:j0 + m], m)
        amp = float(np.prod(1.0 + np.abs(g)))
        for j in range(m):
            tol_h[j0 + j] = 1e-13 * float((np.abs(P[j0 + j].astype(LD)) * absw).sum()) * amp
    tol_w = 1e-13 * absw.astype(float) + (tol_h[:, None] * np.abs(P)).sum(axis=0)
    return tol_h, tol_w


def check_step(P, rows, w):
    h, wn, nrm2, _ = blocked_step(P, rows, w)
    h_ref, w_ref = chain_step(P, w)
    tol_h, tol_w = step_bounds(P, rows, w)
    eh = np.abs(h.astype(LD) - h_ref).astype(float)
    ew = np.abs(wn.astype(LD) - w_ref).astype(float)
    assert np.all(eh <= tol_h), ("h", float((eh / tol_h).max()))
    assert np.all(ew <= tol_w), ("w", float((ew / tol_w).max()))
    t = float((w_ref * w_ref).sum())
    assert abs(nrm2 - t) <= 1e-13 * t + 2.0 * float((np.abs(w_ref).astype(float) * tol_w).sum())


@pytest.mark.parametrize("i", [1, 7, 8, 9, 16, 17, 20])
def test_blocked_step_equals_chain_on_a_skewed_basis(i):
    rng = np.random.default_rng(40 + i)
    P, rows = skewed_basis(rng, i, 257)
    G = P @ P.T - np.eye(i)
    if i > 1:
        assert 0.01 < np.abs(G).max() < 0.2  # far from orthogonal
    w = rng.standard_normal(257)
    check_step(P, rows, w)


@pytest.mark.parametrize("i", [7, 8, 9, 16, 17, 20])
def test_without_the_gram_data_the_check_fails(i):
    """negative control: the raw inner products alone (classical Gram-Schmidt inside a block) miss the bound"""
    rng = np.random.default_rng(40 + i)
    P, rows = skewed_basis(rng, i, 257)
    w = rng.standard_normal(257)
    zeroed = rows.copy()
    zeroed[:, :B] = 0.0
    with pytest.raises(AssertionError):
        check_step(P, zeroed, w)


def test_gram_row_of_the_new_vector():
    """the last pass leaves <p_a, w_final> for the members of the new vector's own block: the row the next steps use"""
    rng = np.random.default_rng(7)
    P, rows = skewed_basis(rng, 11, 129)
    w = rng.standard_normal(129)
    _, wn, nrm2, sums = blocked_step(P, rows, w)
    for a in range(3):
        t = (P[8 + a].astype(LD) * wn.astype(LD)).sum()
        assert abs(sums[a] - float(t)) <= 1e-13 * float(np.abs(P[8 + a] * wn).sum())
    assert np.all(sums[3:B] == 0.0) and sums[B] == nrm2
