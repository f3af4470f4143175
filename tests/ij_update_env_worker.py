"""Update rounds of an IJ matrix in a process of its own, for the switches that are read once per process
(tests/test_gpu_ij_update.py).  Modes:
  stale  GMRES(20) + BoomerAMG set up on A1 = convection_diffusion_3d(12); A1 updated to A2 = 3 A1 + diag(seeded values
         in [0, 1]) from device arrays; a solve without a new Setup (true residual by scipy), then Setup again on the same
         handles against fresh handles on a fresh A2: level operators bit for bit, iteration counts, solutions.
  round  one device update round of the 16^3 7-point system and a GMRES + BoomerAMG solve; a digest of everything.
Prints one RESULT line of JSON."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from tests import ij_cases as cases  # noqa: E402
from tests import ij_update_cases as upd  # noqa: E402


def solvers(mi, tol):
    amg = mi.BoomerAMG(print_level=0)
    gm = mi.GMRES(tolerance=tol, max_iterations=200, kspace=20, print_level=0)
    gm.set_precond(amg)
    return amg, gm


def levels(amg):
    out = []
    for l in range(amg.num_levels):
        for w in (0, 2, 3):
            if w and l == amg.num_levels - 1:
                continue
            ia, ja, a, shape = amg.level_csr(l, w)
            out.append((ia, ja, a.view(np.int64), np.array(shape)))
    return out


def stale(mi):
    from tests.systems import convection_diffusion_3d

    A1 = convection_diffusion_3d(12).tocoo()
    N = A1.shape[0]
    r, c, v = A1.row.astype(np.int64), A1.col.astype(np.int64), A1.data.astype(np.float64)
    shift = np.random.default_rng(41).uniform(0.0, 1.0, size=N)
    v2 = 3.0 * v + np.where(r == c, shift[r], 0.0)
    A2 = A1.tocsr() * 3.0
    A2.setdiag(A2.diagonal() + shift)
    bv = np.cos(np.arange(N, dtype=np.float64))
    A = cases.new_matrix(mi, 0, N - 1)
    cases.stage(mi, A, [(r, c, v, False)], True)
    A.assemble()
    b, x = mi.IJVector(0, N - 1, bv), mi.IJVector(0, N - 1, np.zeros(N))
    amg, gm = solvers(mi, 1e-9)
    gm.setup(A, b, x)
    assert gm.solve(A, b, x) == 0
    # the update: zero, then the new values added, as a time-stepping caller does
    upd.apply_round(mi, A, [("const", 0.0), (r, c, v2, True)], device=True)
    x.set(np.zeros(N))
    assert gm.solve(A, b, x) == 0
    stale_iters = gm.num_iterations
    true_rel = float(np.linalg.norm(bv - A2 @ x.get()) / np.linalg.norm(bv))
    # Setup again on the same handles / fresh handles on a fresh matrix
    gm.setup(A, b, x)
    x.set(np.zeros(N))
    assert gm.solve(A, b, x) == 0
    again = (gm.num_iterations, levels(amg), x.get().view(np.int64))
    F = cases.new_matrix(mi, 0, N - 1)
    cases.stage(mi, F, [(r, c, v2, False)], False)
    F.assemble()
    xf = mi.IJVector(0, N - 1, np.zeros(N))
    amg2, gm2 = solvers(mi, 1e-9)
    gm2.setup(F, b, xf)
    assert gm2.solve(F, b, xf) == 0
    fresh = (gm2.num_iterations, levels(amg2), xf.get().view(np.int64))
    eq = len(again[1]) == len(fresh[1]) and all(
        all(p.shape == q.shape and np.array_equal(p, q) for p, q in zip(s, t)) for s, t in zip(again[1], fresh[1]))
    return {"stale_iters": stale_iters, "stale_true_rel_res": true_rel, "levels": amg.num_levels, "levels_equal": bool(eq),
            "resetup_iters": again[0], "fresh_iters": fresh[0], "x_equal": bool(np.array_equal(again[2], fresh[2]))}


def one_round(mi):
    n = 16
    N = n ** 3
    r, c, v = cases.laplace_triples(mi, n, 7)
    p = np.random.default_rng(5).permutation(len(v))
    A = cases.new_matrix(mi, 0, N - 1)
    cases.stage(mi, A, [(r, c, v, False)], True)
    A.assemble()
    v2 = 2.0 * v + np.where(r == c, 0.25, 0.0)
    upd.apply_round(mi, A, [("const", 0.0), (r[p].copy(), c[p].copy(), v2[p].copy(), True)], device=True)
    snap = cases.snapshot(mi, A)
    b, x = mi.IJVector(0, N - 1, np.cos(np.arange(N, dtype=np.float64))), mi.IJVector(0, N - 1, np.zeros(N))
    amg, gm = solvers(mi, 1e-9)
    gm.setup(A, b, x)
    assert gm.solve(A, b, x) == 0
    h = hashlib.sha256()
    for k in sorted(snap):
        h.update(np.ascontiguousarray(snap[k]).tobytes())
    h.update(x.get().tobytes())
    h.update(gm.residual_history().tobytes())
    return {"digest": h.hexdigest(), "iters": gm.num_iterations, "device_value_updates": mi.counter("ij_device_value_updates")}


def main():
    mi = ge.load_binding()
    mi.init()
    print("RESULT " + json.dumps(stale(mi) if sys.argv[1] == "stale" else one_round(mi)))


if __name__ == "__main__":
    main()
