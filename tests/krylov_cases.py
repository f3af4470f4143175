"""The case table of the Krylov control-path tests, shared by tests/test_krylov_spec.py (restatement against the CPU
oracle, and the conditions that keep every case away from a coin-flip at its tolerance) and
tests/test_gpu_krylov_paths.py (the device loops against the restatement).

A case is a dict: id, op (operator name), b / x0 (how the vectors are made), the solver arguments (tol, atol,
max_iter, min_iter, kdim, two_norm), amg (preconditioned by the default BoomerAMG, tabulated as a dense map for the
restatement) and ncomp.  `system(case)` builds (scipy A, b, x0); solver families are listed per group."""
import numpy as np
import scipy.sparse as sp

from tests.systems import convection_diffusion_3d

GMRES_FAMILY = ("gmres", "fgmres", "cogmres1", "cogmres2")
ALL_SOLVERS = GMRES_FAMILY + ("pcg", "bicgstab")

_OPS = {}


def operator(name):
    """cd7 / cd9: the non-symmetric convection-diffusion operator on 7^3 = 343 / 9^3 = 729 points (both odd);
    lap7: the 7-point Laplacian on 7^3; two_i: 2 I; diag3: diag(1, 2, 4, 1, 2, 4, ...) -- three eigenvalues;
    skew: the antisymmetric tridiagonal (+1 above, -1 below the diagonal), <r, A r> = 0 for every r."""
    if name not in _OPS:
        n = 343
        if name == "cd7":
            M = convection_diffusion_3d(7)
        elif name == "cd9":
            M = convection_diffusion_3d(9)
        elif name == "lap7":
            T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(7, 7))
            I = sp.identity(7)
            M = sp.kron(sp.kron(T, I), I) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(I, I), T)
        elif name == "two_i":
            M = 2.0 * sp.identity(n)
        elif name == "diag3":
            M = sp.diags(np.tile([1.0, 2.0, 4.0], n // 3 + 1)[:n])
        elif name == "skew":
            M = sp.diags([-1.0, 1.0], [-1, 1], shape=(n, n))
        else:
            raise KeyError(name)
        M = M.tocsr()
        M.sort_indices()
        _OPS[name] = M
    return _OPS[name]


def system(case):
    """(A scipy csr, b, x0) of a case; multi-component vectors are component-major (ncomp, n).
    b kinds: "Ax" A times a seeded random vector, "zero", "nan" (Ax with one NaN), "2x0" (exact guess on 2 I),
    "unit" (4 e_17: every operation of the first Arnoldi step on 2 I is exact, the new basis vector is 0),
    "ints" (small integers: <r0, A r0> on the skew operator is exactly 0 in any summation order).
    x0 kinds: "rand" (the same generator, after b's vector), "zero"."""
    A = operator(case["op"])
    n, nc = A.shape[0], case.get("ncomp", 1)
    rng = np.random.default_rng(3)
    xs = rng.standard_normal((nc, n))
    x0 = rng.standard_normal((nc, n)) if case["x0"] == "rand" else np.zeros((nc, n))
    kind = case["b"]
    if kind in ("Ax", "nan"):
        b = np.stack([A @ v for v in xs])
        if kind == "nan":
            b[nc - 1, n // 2] = np.nan
    elif kind == "zero":
        b = np.zeros((nc, n))
    elif kind == "2x0":
        b = 2.0 * x0
    elif kind == "unit":
        b = np.zeros((nc, n))
        b[:, 17] = 4.0
    elif kind == "ints":
        b = np.stack([np.rint(3.0 * v) for v in xs])
    else:
        raise KeyError(kind)
    if nc == 1:
        return A, b[0], x0[0]
    return A, b, x0


def make_case(id, op, b="Ax", x0="rand", **kw):
    d = dict(id=id, op=op, b=b, x0=x0, tol=1e-9, atol=0.0, max_iter=200, min_iter=0, kdim=20, two_norm=0, amg=False,
             ncomp=1)
    d.update(kw)
    return d


_c = make_case

# Tolerances: 1e-9 / 1e-10 and atol 1e-3 unless a case needs another one to keep every tested estimate outside
# (0.9, 1.1) eps (test_krylov_spec.py condition b).  With b = 0 the solution is 0 and x is what is left of x0 after
# cancellation: its error is u * cond * |x0| whatever the tolerance, so those cases stop at 1e-2, where x is still
# large enough for the relative bound on x to mean something.
# ---- no preconditioner, n = 343: GMRES, FlexGMRES, COGMRES cgs 1 and cgs 2 (the same Krylov space, one restatement)
# MIN_ITER_OWN: tol 1e-2 is met after this many iterations (pinned by the spec test); the case asks for four more
MIN_ITER_OWN = 6
NOPRECOND = [
    _c("converge_k20", "cd7"),                        # 40 iterations, two cycles that fill all 20 basis vectors
    _c("restart_k5_cap60", "cd7", kdim=5, max_iter=60),  # max_iter at the end of a cycle, code 256
    _c("cap17_midcycle", "cd7", max_iter=17),         # max_iter inside a cycle: x from a partial basis, code 256
    _c("b_zero", "cd7", b="zero", tol=1e-2),          # den = ||r0||; the solution is 0: see the note above
    _c("atol", "cd7", tol=0.0, atol=1e-3),
    _c("min_iter", "cd7", tol=1e-2, min_iter=MIN_ITER_OWN + 4),
    _c("nan_in_b", "cd7", b="nan"),                   # code 1, no iteration, x untouched
]

# ---- exact and degenerate systems, n = 343
DEGENERATE = [
    _c("two_i", "two_i"),                             # one step; the next basis vector is rounding noise
    _c("exact_guess", "two_i", b="2x0"),              # r0 = 0 exactly
    _c("three_eigenvalues", "diag3"),                 # three steps
]
LUCKY = _c("lucky_breakdown", "two_i", b="unit", x0="zero")   # GMRES family: the new basis vector is exactly 0

BICGSTAB = [
    _c("bicgstab_x0", "cd7", tol=1e-8),
    _c("bicgstab_b_zero", "cd7", b="zero", tol=1e-2),
    _c("bicgstab_cap3", "cd7", max_iter=3),
    _c("bicgstab_atol", "cd7", tol=0.0, atol=1e-3),
    _c("bicgstab_breakdown", "skew", b="ints", x0="zero"),   # <r0, A p> = 0: leaves the loop in iteration 1, code 0
    _c("bicgstab_nan_in_b", "cd7", b="nan"),
]

PCG = [
    _c("pcg_x0", "lap7", tol=3e-9),
    _c("pcg_two_norm", "lap7", tol=3e-9, two_norm=1),
    _c("pcg_atol", "lap7", tol=0.0, atol=2e-3),
    _c("pcg_b_zero", "lap7", b="zero"),               # x = 0 exactly, no iteration, code 0
    _c("pcg_nan_in_b", "lap7", b="nan"),
]
PCG_AMG = [dict(c, id=c["id"] + "_amg", amg=True) for c in PCG[:4]]

# ---- BoomerAMG-preconditioned, n = 729, x0 != 0: (solver, case)
AMG = [
    ("gmres", _c("amg_gmres_k3", "cd9", tol=1e-10, kdim=3, amg=True)),
    ("gmres", _c("amg_gmres_k50", "cd9", tol=1e-10, kdim=50, amg=True)),
    ("fgmres", _c("amg_fgmres_k3", "cd9", tol=1e-10, kdim=3, amg=True)),
    ("bicgstab", _c("amg_bicgstab", "cd9", tol=1e-10, amg=True)),
]

# ---- three components, a random x0 per component
MULTI = []
for _op in ("cd7", "cd9"):
    MULTI += [
        ("gmres", _c(f"multi_{_op}_gmres_k5", _op, kdim=5, max_iter=60, ncomp=3)),
        ("gmres", _c(f"multi_{_op}_gmres_amg", _op, tol=1e-10, amg=True, ncomp=3)),
        ("bicgstab", _c(f"multi_{_op}_bicgstab_amg", _op, tol=1e-10, amg=True, ncomp=3)),
    ]


def all_cases():
    """every (solver, case) of the table"""
    out = [(s, c) for c in NOPRECOND for s in GMRES_FAMILY]
    out += [(s, c) for c in DEGENERATE for s in ALL_SOLVERS]
    out += [(s, LUCKY) for s in GMRES_FAMILY]
    out += [("bicgstab", c) for c in BICGSTAB]
    out += [("pcg", c) for c in PCG + PCG_AMG]
    out += AMG + MULTI
    return out


def case_id(sc):
    return f"{sc[0]}-{sc[1]['id']}"


def reference(solver, case, A, b, x0, M=None):
    """the restatement's answer for a case; M: the preconditioner as a callable on one component (None: identity)"""
    from tests import krylov_ref as kr

    nc = case.get("ncomp", 1)
    Ad = kr.block_operator(A.toarray(), nc)
    kw = dict(x0=np.ravel(x0), M=kr.per_component(M, nc), tol=case["tol"], atol=case["atol"],
              max_iter=case["max_iter"], min_iter=case["min_iter"])
    if solver == "pcg":
        return kr.pcg(Ad, np.ravel(b), two_norm=case["two_norm"], **kw)
    if solver == "bicgstab":
        return kr.bicgstab(Ad, np.ravel(b), **kw)
    return kr.gmres(Ad, np.ravel(b), kdim=case["kdim"], flexible=(solver == "fgmres"), **kw)
