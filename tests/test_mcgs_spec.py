"""CPU: the multicolour Gauss-Seidel smoother (relax types 40 / 41 / 42) as far as it goes without
a device -- the names of the ABI and of the binding, the refusals of the host-only setup and of more than one rank, the
instantiations of the in-place pass, and the numpy restatement (tests/mcgs_ref.py) against scipy's triangular solves."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests import mcgs_cases as cases
from tests import mcgs_ref as ref
from tests.agg2s_common import host_amg, ij_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_names_exist(mi_lib):
    text = open(os.path.join(ROOT, "include", "HYPRE_mi_ext.h")).read()
    assert re.search(r"HYPRE_Int\s+HYPRE_MI_BoomerAMGGetLevelColours\s*\(", text)
    assert hasattr(mi_lib.lib(), "HYPRE_MI_BoomerAMGGetLevelColours")
    assert callable(mi_lib.BoomerAMG.level_colours)
    assert mi_lib.PROF_LVL_RELAX_MC == mi_lib.PROF_LVL_RELAX0 + 16
    assert "40 / 41 / 42" in open(os.path.join(ROOT, "include", "HYPRE_parcsr_ls.h")).read()


@pytest.mark.parametrize("slot", ["all", "down", "up", "coarse"])
@pytest.mark.parametrize("t", [40, 41, 42])
def test_host_only_setup_refuses_by_name(mi_lib, t, slot):
    mi = mi_lib
    kw = dict(relax_type=t) if slot == "all" else dict(
        down_relax_type=t if slot == "down" else 8, up_relax_type=t if slot == "up" else 8,
        coarse_relax_type=t if slot == "coarse" else 9)
    with pytest.raises(mi.HypreError, match=r"relax_type %d \(multicolour Gauss-Seidel\) is not implemented by the "
                                            r"host-only setup \(the colouring is device code\)" % t):
        host_amg(mi, ij_host(mi, cases.case("lap7_6")), **kw)
    mi.call("HYPRE_ClearAllErrors")


def test_unknown_relax_type_names_the_new_ones(mi_lib):
    mi = mi_lib
    with pytest.raises(mi.HypreError, match=r"relax_type 43 is not implemented \(.*16, 18, 40, 41, 42 are\)"):
        host_amg(mi, ij_host(mi, cases.case("lap7_6")), relax_type=43)
    mi.call("HYPRE_ClearAllErrors")


def test_in_place_pass_has_an_instantiation_for_every_value_format(mi_lib):
    pick = mi_lib.solve_kernel_choice
    names = set()
    for xcache, tile in ((False, 2048), (True, 2048), (True, 4096)):
        for fp32, dictionary in ((False, False), (True, False), (False, True)):
            if dictionary and not xcache:
                continue  # (the plain stream has no dictionary form)
            name = pick(0, xcache=xcache, tile_entries=tile, fp32=fp32, dictionary=dictionary, epilogue=3)
            assert re.match(r"spmv_stream(_xc)?<3, 0", name), name
            assert name != pick(0, xcache=xcache, tile_entries=tile, fp32=fp32, dictionary=dictionary, epilogue=1)
            names.add(name)
    assert len(names) == 8


@pytest.mark.parametrize("name", ["lap7_6", "mixed700", "unsymmetric"])
@pytest.mark.parametrize("omega", [1.0, 0.8])
def test_restatement_equals_the_triangular_solves(name, omega):
    """u + omega (D + omega L)^-1 (f - A u) forward, with U backward: the splitting form of the sweep, by scipy's
    triangular solve.  Tolerance: 1e-12 x max|u| -- both sides are float64 substitutions of a diagonally dominant
    operator that round in another order (measured: below 4e-15)."""
    A = cases.case(name)
    n = A.shape[0]
    rng = np.random.default_rng(1)
    u, f = rng.standard_normal(n), rng.standard_normal(n)
    D = sp.diags(A.diagonal())
    lower, upper = sp.tril(A, -1), sp.triu(A, 1)

    def step(v, T):
        return v + omega * spla.spsolve_triangular((D + omega * T).tocsr(), f - A @ v, lower=T is lower)

    want = {ref.FORWARD: step(u, lower), ref.BACKWARD: step(u, upper), ref.SYMMETRIC: step(step(u, lower), upper)}
    for d, w in want.items():
        got = ref.sweep(A, u, f, omega, d)
        assert np.abs(got - w).max() <= 1e-12 * np.abs(w).max(), (d, np.abs(got - w).max())
        wide = ref.sweep(A, u, f, omega, d, dtype=np.longdouble)
        assert np.abs(got - wide.astype(np.float64)).max() <= 1e-13 * np.abs(w).max()


def test_rows_of_one_colour_may_be_swept_in_any_order():
    """the 7-point operator in red-black order: the sequential sweep gives the same bits however the rows of one colour
    are permuted among themselves -- what lets a colour pass run its rows in parallel"""
    n = 6
    A = cases.case("lap7_6")
    idx = np.arange(n ** 3)
    colour = ((idx % n) + (idx // n) % n + idx // (n * n)) % 2
    assert not ref.colouring_conflicts(A, colour)
    order = np.argsort(colour, kind="stable")
    B = A[order][:, order].tocsr()
    rng = np.random.default_rng(2)
    u, f = rng.standard_normal(n ** 3), rng.standard_normal(n ** 3)
    nred = int((colour == 0).sum())
    for d in (ref.FORWARD, ref.BACKWARD, ref.SYMMETRIC):
        base = ref.sweep(B, u, f, 0.8, d)
        for seed in (3, 4):
            r = np.random.default_rng(seed)
            shuffled = np.concatenate([r.permutation(nred), nred + r.permutation(n ** 3 - nred)])
            assert np.array_equal(ref.sweep(B, u, f, 0.8, d, order=shuffled), base)
    # and a conflict is found where there is one
    colour[1] = colour[0]
    assert ref.colouring_conflicts(A, colour)


def test_more_than_one_rank_is_refused():
    env = dict(os.environ, MI_HYPRE_HOST_THREADS="2", OMP_NUM_THREADS="1", MI_HYPRE_LOCALITY_ORDER="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", "30991", os.path.join(ROOT, "tests", "mcgs_dist_worker.py")]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    assert p.stdout.count("mcgs rank ok") == 2, p.stdout[-4000:]
