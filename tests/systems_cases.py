"""Inputs of the unknown-based systems AMG tests (num_functions, dof_func; DESIGN.md section 3, "Systems of PDEs"):
small coupled PDE systems with the unknown every row belongs to.  Everything is generated from fixed numbers and seeds.
Shared by tests/test_systems_amg_spec.py, tests/test_gpu_systems_amg.py and tests/systems_worker.py."""
import numpy as np
import scipy.sparse as sp

THETA = 0.25  # strong threshold of every hierarchy of these tests


def _d2(n):
    return sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n)).tocsr()


def _d1(n):
    return sp.diags([-0.5, 0.5], [-1, 1], shape=(n, n)).tocsr()


def _axis(ops, axis, n):
    """the 1-D operators `ops[axis]` along their axis of an n^3 grid, the identity along the others (x fastest)"""
    I = sp.identity(n, format="csr")
    m = [ops.get(a, I) for a in (2, 1, 0)]  # kron order: z, y, x
    return sp.kron(sp.kron(m[0], m[1]), m[2]).tocsr()


def interleave(blocks, k):
    """the k x k block matrix (function-major: unknown a of node p is row a * nodes + p) renumbered so that the unknowns
    of a node are consecutive (row p * k + a)"""
    M = sp.bmat(blocks, format="csr")
    nodes = M.shape[0] // k
    new = np.arange(M.shape[0])
    old = (new % k) * nodes + new // k
    M = M[old][:, old].tocsr()
    M.sort_indices()
    return M


def lame(n=9, lam=1.0, mu=1.0, interleaved=True):
    """-mu Lap u - (lam + mu) grad div u on an n^3 grid by second-order finite differences, homogeneous Dirichlet
    boundaries, unit spacing: 7 entries of the row's own component and 4 of each of the two others (the mixed second
    derivatives), 15 per interior row.  Symmetric positive definite (smallest eigenvalue 0.46 at n = 9, lam = mu = 1)."""
    d2 = [_axis({a: _d2(n)}, a, n) for a in range(3)]
    d1 = [_axis({a: _d1(n)}, a, n) for a in range(3)]
    lap = d2[0] + d2[1] + d2[2]
    blocks = [[None] * 3 for _ in range(3)]
    for a in range(3):
        for b in range(3):
            blocks[a][b] = mu * lap + (lam + mu) * d2[a] if a == b else -(lam + mu) * (d1[a] @ d1[b])
    if interleaved:
        return interleave(blocks, 3), np.arange(3 * n ** 3, dtype=np.int32) % 3
    M = sp.bmat(blocks, format="csr")
    M.sort_indices()
    return M, (np.arange(3 * n ** 3) // n ** 3).astype(np.int32)


def diffusion_fields(n, k, c, interleaved=True):
    """k diffusion fields on an n^3 grid (7-point, Dirichlet), field a with the diffusivities (1 + a, 1, 1 / (1 + a))
    along x, y, z, every pair of fields coupled at every node by the exchange term c (u_a - u_b)"""
    blocks = [[None] * k for _ in range(k)]
    I = sp.identity(n ** 3, format="csr")
    for a in range(k):
        L = (1.0 + a) * _axis({0: _d2(n)}, 0, n) + _axis({1: _d2(n)}, 1, n) + _axis({2: _d2(n)}, 2, n) / (1.0 + a)
        for b in range(k):
            blocks[a][b] = L + c * (k - 1) * I if a == b else -c * I
    if interleaved:
        return interleave(blocks, k), np.arange(k * n ** 3, dtype=np.int32) % k
    M = sp.bmat(blocks, format="csr")
    M.sort_indices()
    return M, (np.arange(k * n ** 3) // n ** 3).astype(np.int32)


def shuffled(M, dof, seed):
    """the same system with its rows (and columns) in a seeded random order: dof_func is no pattern of the row number"""
    order = np.random.default_rng(seed).permutation(M.shape[0])
    S = M[order][:, order].tocsr()
    S.sort_indices()
    return S, np.ascontiguousarray(dof[order])


# name -> (matrix, dof_func, num_functions, whether dof_func is the interleaved default)
def case(name):
    if name == "lame1":
        return lame(9, 1.0, 1.0) + (3, True)
    if name == "lame10":
        return lame(9, 10.0, 1.0) + (3, True)
    if name == "diff2_weak":
        return diffusion_fields(10, 2, 0.1) + (2, True)
    if name == "diff2_strong":
        return diffusion_fields(10, 2, 10.0) + (2, True)
    if name == "diff3":
        return diffusion_fields(8, 3, 0.1) + (3, True)
    if name == "lame1_major":  # function-major numbering: dof_func through SetDofFunc
        return lame(9, 1.0, 1.0, interleaved=False) + (3, False)
    if name == "diff3_random":  # a seeded random numbering: dof_func through SetDofFunc
        return shuffled(*diffusion_fields(8, 3, 0.1), seed=7) + (3, False)
    raise KeyError(name)


CASES = ("lame1", "lame10", "diff2_weak", "diff2_strong", "diff3", "lame1_major", "diff3_random")

# the settings the hierarchies are compared under (BoomerAMG keyword arguments besides num_functions / dof_func)
SETTINGS = {
    "interp6": dict(interp_type=6, true_pmax_elmts=4),
    "interp0": dict(interp_type=0, true_pmax_elmts=4),
    "interp17": dict(interp_type=17, true_pmax_elmts=4),
    "interp100": dict(interp_type=100),
    "interp4": dict(interp_type=4, true_pmax_elmts=4),
    "falgout": dict(coarsen_type=6, interp_type=6, true_pmax_elmts=4),
    "agg4": dict(agg_num_levels=1, agg_interp_type=4, interp_type=6, true_pmax_elmts=4),
    "agg5": dict(agg_num_levels=1, agg_interp_type=5, interp_type=6, true_pmax_elmts=4),
}


def amg_kwargs(setting, k, dof, default_dof):
    kw = dict(SETTINGS[setting], strong_threshold=THETA, num_functions=k)
    if not default_dof:
        kw["dof_func"] = dof
    return kw
