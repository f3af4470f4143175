"""GPU: unknown-based systems AMG (num_functions, dof_func; DESIGN.md section 3, "Systems of PDEs").  The same-function
filter kernel against numpy bit for bit on every row shape that takes another path; device hierarchies against the
host-only ones bit for bit (a child process per configuration, tests/systems_worker.py); the internal numbering;
GMRES + AMG against the oracle's solve phase on the product's own hierarchy; the driver key."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from tests import systems_cases as sc
from tests import systems_ref as ref
from tests.agg2s_common import csr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "hypre-mini-app_amd", "hypre_app")
WORKER = os.path.join(ROOT, "tests", "systems_worker.py")


def assert_filter_is_numpys(mi, M, dof):
    ia, ja, a, shape = mi.same_function_filter_op(M, dof)
    F = ref.filter_same_function(M, dof)
    assert shape == F.shape and np.array_equal(ia, F.indptr) and np.array_equal(ja, F.indices)
    assert np.array_equal(a.view(np.int64), F.data.view(np.int64))
    return F


def rows_of_lengths(lengths, no_diag_every=3, seed=1):
    """row i holds lengths[i] consecutive columns (modulo n) around its diagonal, placed by a seeded offset; every
    no_diag_every-th row starts right after its diagonal instead and stores none"""
    n = len(lengths)
    assert max(lengths) < n
    rng = np.random.default_rng(seed)
    indptr, indices = [0], []
    for i, ln in enumerate(lengths):
        start = i + 1 if (no_diag_every and i % no_diag_every == 0) else i - int(rng.integers(0, ln))
        indices.append(np.sort((start + np.arange(ln)) % n))
        indptr.append(indptr[-1] + ln)
    indices = np.concatenate(indices).astype(np.int64)
    return sp.csr_matrix((rng.standard_normal(len(indices)), indices, np.array(indptr)), shape=(n, n))


def row_group(M):
    """lanes per row as the library chooses them: the power of two next to two thirds of the mean row length"""
    g, avg = 1, M.nnz / M.shape[0]
    while g < 64 and g * 1.5 < avg:
        g *= 2
    return g


# lanes per row G -> (length, number) of the filler rows that bring the mean row length of a matrix holding one row of
# every length 1 ... 130 (mean 65.5: G = 64) down to where the library picks G
FILLER = {1: (1, 20832), 2: (2, 16380), 4: (4, 7865), 8: (9, 7215), 16: (18, 2958), 32: (36, 829), 64: (70, 40)}
_group_matrix = {}


def group_matrix(G):
    if G not in _group_matrix:
        f, nf = FILLER[G]
        rng = np.random.default_rng(G)
        lengths = np.array(list(range(1, 131)) + [f] * nf)
        M = rows_of_lengths(rng.permutation(lengths).tolist(), seed=G)
        assert row_group(M) == G and set(range(1, 131)) <= set(np.diff(M.indptr).tolist())
        _group_matrix[G] = M
    return _group_matrix[G]


def test_filter_kernel_one_row(mi):
    for M in (sp.csr_matrix(np.array([[2.5]])), sp.csr_matrix((1, 1))):
        F = assert_filter_is_numpys(mi, M, np.zeros(1, dtype=np.int32))
        assert F.nnz == M.nnz


@pytest.mark.parametrize("k", [1, 2, 3, 7])
@pytest.mark.parametrize("G", sorted(FILLER))
def test_filter_kernel_every_lane_group_rows_of_every_length_1_to_130(mi, G, k):
    """for every number of lanes per row the library can pick: rows of every length 1 ... 130 -- shorter and longer
    than the group, more than one batch per group, longer than a wave --, every third row without a stored diagonal,
    more than one block, a seeded random dof_func"""
    M = group_matrix(G)
    dof = np.random.default_rng(1000 + k).integers(0, k, size=M.shape[0]).astype(np.int32)
    F = assert_filter_is_numpys(mi, M, dof)
    assert (k > 1) == (F.nnz < M.nnz)
    assert M.shape[0] * G > 256  # more than one block


def test_filter_kernel_rows_that_keep_only_the_diagonal_or_nothing(mi):
    M = group_matrix(64).tolil()
    n = M.shape[0]
    dof = np.random.default_rng(5).integers(0, 3, size=n).astype(np.int32)
    # a row whose only kept entry is the diagonal: every other column belongs to another function
    cols40 = sorted(set(np.flatnonzero(dof != dof[40])[:25].tolist()) | {40})
    M.rows[40], M.data[40] = cols40, [1.0] * len(cols40)
    # a row without a stored diagonal whose entries all go
    M.rows[41], M.data[41] = sorted(np.flatnonzero(dof != dof[41])[:7].tolist()), [2.0] * 7
    M = M.tocsr()
    M.sort_indices()
    F = assert_filter_is_numpys(mi, M, dof)
    assert F.indptr[41] - F.indptr[40] == 1 and F.indices[F.indptr[40]] == 40
    assert F.indptr[42] == F.indptr[41]


@pytest.mark.parametrize("name", ["lame1", "diff3_random"])
def test_filter_kernel_on_the_systems(mi, name):
    M, dof, k, _ = sc.case(name)
    assert_filter_is_numpys(mi, M, dof)


def run_worker(*args, **env):
    e = dict(os.environ, MI_HYPRE_DEVICE_SETUP_MIN_ROWS="0", MI_HYPRE_LOCALITY_ORDER="0")
    e.update({k: str(v) for k, v in env.items()})
    p = subprocess.run([sys.executable, WORKER] + list(args), env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])


_plain = {}


@pytest.mark.parametrize("setting", ["interp6", "interp0", "interp17", "interp100", "agg5"])
@pytest.mark.parametrize("name", ["lame10", "diff3"])
def test_device_hierarchy_has_the_bits_of_the_host_only_one(name, setting):
    r = run_worker("hierarchy", name, setting)
    assert r["levels"] >= 3 and r["rows"][0] == sc.case(name)[0].shape[0]
    _plain[name, setting] = r


def test_device_hierarchy_reads_no_memory_it_has_not_written():
    r = run_worker("hierarchy", "lame10", "interp6", MI_HYPRE_POISON_ALLOC=1)
    base = _plain.get(("lame10", "interp6")) or run_worker("hierarchy", "lame10", "interp6")
    assert r == base


def test_dof_func_follows_the_internal_numbering_and_the_solve_converges():
    r = run_worker("locality", "lame1_major", MI_HYPRE_LOCALITY_ORDER=1)
    assert r["levels"] >= 3 and 0 < r["iters"] < 60


def chunk_of(mi):
    c = mi.c_int()
    mi.call("HYPRE_MI_GetGSChunk", mi.C.byref(c))
    return c.value


def test_gmres_amg_matches_the_oracle_on_the_products_hierarchy(mi, oc):
    """Lame 9^3, lambda = 10: the residual history of GMRES + AMG (num_functions 3) against the oracle's GMRES with the
    oracle's solve phase on the product's own levels (from_levels); the bars of tests/test_gpu_amg.py for that
    comparison: same iteration count, 1e-8 relative per step, final relative residual within 1e-10"""
    from tests.systems_worker import device_matrix

    M, dof, k, _ = sc.case("lame10")
    n = M.shape[0]
    A = device_matrix(mi, M)
    rhs = M @ np.ones(n)
    b, x = mi.IJVector(0, n - 1, rhs), mi.IJVector(0, n - 1, np.zeros(n))
    amg = mi.BoomerAMG(print_level=0, num_functions=3, strong_threshold=sc.THETA)
    gm = mi.GMRES(tolerance=1e-8, max_iterations=100, kspace=50, print_level=0)
    gm.set_precond(amg)
    gm.setup(A, b, x)
    assert gm.solve(A, b, x) == 0
    nl = amg.num_levels
    assert nl >= 3
    As = [oc.Csr.from_scipy(csr(amg, l, 0)) for l in range(nl)]
    Ps = [oc.Csr.from_scipy(csr(amg, l, 2)) for l in range(nl - 1)]
    oamg = oc.Amg.from_levels(As, Ps, [amg.level_cf(l) for l in range(nl - 1)],
                              oc.default_params(gs_chunk=chunk_of(mi), strong_threshold=sc.THETA))
    perm0 = amg.level_perm(0)  # level 0 of the hierarchy is the caller's operator with its rows in this order
    xo, info = oc.gmres(As[0], rhs[perm0], kdim=50, tol=1e-8, maxit=100, amg=oamg)
    hist = gm.residual_history()
    print("iterations %d (oracle %d), final relative residual %.3e (oracle %.3e)" % (gm.num_iterations, info["iters"],
                                                                                   gm.final_rel_res, info["rel_res"]))
    assert gm.num_iterations == info["iters"] and len(hist) == len(info["norms"])
    assert np.allclose(hist, info["norms"], rtol=1e-8, atol=0.0)
    assert abs(gm.final_rel_res - info["rel_res"]) <= 1e-10
    xs = x.get()
    assert np.abs(xs[perm0] - xo).max() < 1e-9 and np.abs(xs - 1.0).max() < 1e-5


def write_mm_matrix(path, A):
    coo = A.tocoo()
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n% written by tests/test_gpu_systems_amg.py\n")
        f.write(f"{A.shape[0]} {A.shape[1]} {coo.nnz}\n")
        for r, c, v in zip(coo.row, coo.col, coo.data):
            f.write(f"{r + 1} {c + 1} {v:.17g}\n")


def write_mm_vector(path, v):
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix array real general\n% vector\n")
        f.write(f"{len(v)} 1\n")
        for x in v:
            f.write(f"{x:.17g}\n")


def test_driver_key_num_functions(mi, tmp_path):
    """hypre_app on a MatrixMarket file with boomeramg_settings: num_functions 3: the iteration count of the Python
    path, and the per-level line reports the rows per function"""
    from tests.systems_worker import device_matrix

    M, dof, k, _ = sc.case("lame10")
    n = M.shape[0]
    rhs = M @ np.ones(n)
    write_mm_matrix(tmp_path / "mat.mm", M)
    write_mm_vector(tmp_path / "rhs.mm", rhs)
    write_mm_vector(tmp_path / "sln.mm", np.ones(n))
    (tmp_path / "input.yaml").write_text("""
linear_system:
  type: matrix_market
  matrix_file: mat.mm
  rhs_file: rhs.mm
  sln_file: sln.mm
  write_outputs: false
  rtol: 1.0e-5
  atol: 1.0e-7

solver_settings:
  method: gmres
  preconditioner: boomeramg
  tolerance: 1.0e-8
  max_iterations: 100
  kspace: 50
  print_level: 0

boomeramg_settings:
  print_level: 1
  strong_threshold: 0.25
  num_functions: 3
""")
    p = subprocess.run([APP, str(tmp_path / "input.yaml")], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    m = re.search(r"Solve 0 : (\d+) iterations", p.stdout)
    assert m and "allClose=1" in p.stdout, p.stdout[-3000:]
    assert re.search(r"level  0: local rows\s+2187 .*rows per function 729 / 729 / 729", p.stdout), p.stdout[-3000:]
    A = device_matrix(mi, M)
    b, x = mi.IJVector(0, n - 1, rhs), mi.IJVector(0, n - 1, np.zeros(n))
    amg = mi.BoomerAMG(print_level=0, num_functions=3, strong_threshold=sc.THETA)
    gm = mi.GMRES(tolerance=1e-8, max_iterations=100, kspace=50, print_level=0)
    gm.set_precond(amg)
    gm.setup(A, b, x)
    assert gm.solve(A, b, x) == 0
    assert gm.num_iterations == int(m.group(1))
    # and without the key the driver builds the scalar hierarchy: no such report
    text = (tmp_path / "input.yaml").read_text().replace("  num_functions: 3\n", "")
    (tmp_path / "input.yaml").write_text(text)
    p = subprocess.run([APP, str(tmp_path / "input.yaml")], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert p.returncode == 0 and "rows per function" not in p.stdout
