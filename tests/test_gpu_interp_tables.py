"""GPU: the device interpolation kernel (sk::interp, interp_group_k) in every table size and in its fallback, on the
operators of tests/systems.py INTERP_TABLE_OPERATORS (what they contain is asserted on the CPU in
tests/test_interp_tables_spec.py): rows whose bound T is a table's capacity and one more at 16 / 17, 32 / 33, 128 / 129,
512 / 513 and 1024, hundreds of rows in the 512- and 1024-entry tables with negative diagonals, special F points, zero
distribution sums, ties in |weight|, classical and ext+i, with and without truncation; and one row over 1024, which
sends the level to the host routine.  HYPRE_MI_BoomerAMGGetInterpCensus says what ran, and the test holds it against the
Python statement of the bound: a change of the binning rule fails here instead of silently moving the rows to other
tables.  Bars: hierarchies bit for bit against the oracle and under negation, as in tests/test_gpu_mixed_sign.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.agg2s_ref import strength_rows
from tests.interp_tables_worker import hierarchy_digest
from tests.systems import INTERP_TABLE_OPERATORS, interp_table_operator
from tests.test_gpu_amg import _chunk
from tests.test_gpu_mixed_sign import assert_mirrored_hierarchies
from tests.test_gpu_setup_kernels import _assert_same_hierarchy
from tests.test_interp_tables_spec import CENSUS_KEYS, bounds, interp_bounds, library_kw, oracle_params, predicted_census

pytestmark = pytest.mark.gpu

SETTINGS = [{}, dict(interp_type=0), dict(trunc_factor=0.2, true_pmax_elmts=0), dict(true_pmax_elmts=2, trunc_factor=0.2),
            dict(true_pmax_elmts=0)]
CASES = [(name, kw) for name in ("dense1200", "dense1600", "hubs", "hubs_ext") for kw in SETTINGS]
# `hubs` was made for classical interpolation (under ext+i its longest rows exceed every table and level 0 falls back,
# which the census must say): the truncation settings once more with it
CASES += [("hubs", dict(kw, interp_type=0)) for kw in SETTINGS[2:]]



def _id(v):
    return "-".join("%s=%s" % kv for kv in v.items()) or "default" if isinstance(v, dict) else v


_operators = {}


def operator(name):
    if name not in _operators:
        _operators[name] = interp_table_operator(name)[0]
    return _operators[name]


def device_setup(mi, name, kw, sign=1):
    M = operator(name)
    A = mi.matrix_from_scipy(M if sign > 0 else (-M).tocsr())
    amg = mi.BoomerAMG(print_level=0, **library_kw(name, kw))
    amg.setup(A)
    return amg


def check_census(amg, want0):
    """level 0 as predicted; every level with a P: the kernel was asked, and its rows are all accounted for -- or none
    is, on a level that fell back; the coarsest level: no interpolation, the host flag"""
    got0 = amg.interp_census(0)
    assert got0 == want0, (got0, want0)
    for l in range(amg.num_levels):
        c = amg.interp_census(l)
        print("census level %d:" % l, c)
        rows = amg.level_csr(l, 0)[3][0]
        if l == amg.num_levels - 1:
            assert c["host"] and not c["fell_back"] and c["max_bound"] == 0 and sum(c[k] for k in CENSUS_KEYS) == 0
            continue
        assert not c["host"], l
        assert sum(c[k] for k in CENSUS_KEYS) == (0 if c["fell_back"] else rows), (l, c)
        assert c["fell_back"] == (c["max_bound"] > 1024), (l, c)
    return got0


@pytest.mark.parametrize("name,kw", CASES, ids=_id)
def test_every_table_equals_oracle_and_census_matches_the_bound(mi, oc, name, kw, monkeypatch):
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    amg = device_setup(mi, name, kw)
    oamg = oc.Amg(oc.Csr.from_scipy(operator(name)), oracle_params(oc, name, kw, gs_chunk=_chunk(mi)))
    assert amg.num_levels > 2
    _assert_same_hierarchy(amg, oamg)
    want = predicted_census(*bounds(oc, name, kw.get("interp_type", 6)))
    got = check_census(amg, want)
    if kw.get("interp_type", 6) == INTERP_TABLE_OPERATORS[name][2]:  # the setting the operator was made for
        assert got["cap512"] >= 4 and (got["cap1024"] >= 4 or name == "dense1200")
    if kw.get("true_pmax_elmts") == 0 and "trunc_factor" not in kw and not got["fell_back"]:
        assert np.diff(amg.level_csr(0, 2)[0]).max() >= 60  # rows of P as long as the interpolatory set


def test_trial_tables_keep_the_rows_that_fit(mi, oc, monkeypatch):
    """the other side of the 33 ... 128 bin (every such row of the operators above is given up by the 32-entry trial and
    rerun): on the 27-point Laplacian of 10^3 points the bound counts 33 to 79 candidates with multiplicity, no row has
    more than 32 distinct ones, and all 643 stay in the trial's tables -- as the Python statement predicts"""
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    Ao = oc.Csr.laplace(10, 10, 10, 27)[0]
    M = Ao.to_scipy().tocsr()
    M.sort_indices()
    amg = mi.BoomerAMG(print_level=0, strong_threshold=0.25)
    amg.setup(mi.matrix_from_scipy(M))
    oamg = oc.Amg(Ao, oc.default_params(strong_threshold=0.25, gs_chunk=_chunk(mi)))
    _assert_same_hierarchy(amg, oamg)
    cf = np.zeros(M.shape[0], dtype=np.int64)
    cf[np.asarray(oamg.level_perm(0))] = np.asarray(oamg.level_cf(0))
    want = predicted_census(*interp_bounds(strength_rows(M, 0.25, 0.9), cf, True))
    assert want["try32_kept"] >= 600 and want["try32_retried"] == 0
    check_census(amg, want)


@pytest.mark.parametrize("name", ["hubs", "hubs_ext"])
def test_long_rows_mirror_under_negation(mi, oc, name, monkeypatch):
    """the device setup of -A against the device setup of A, untruncated and with the default pmax 4, in the
    interpolation the operator was made for: the bar of test_device_setup_mirrors_under_negation -- the same marks, the
    same bits in P and R, A_l negated bit for bit.  One exception, which is arithmetic and not the kernels': with the
    untruncated P a few Galerkin sums of these operators cancel exactly (1 entry of level 1 on hubs, 10 on hubs_ext, in
    the oracle as well), and x + (-x) is +0 for either sign of x.  Entries that are exactly zero on both sides are
    compared as values; there must be as many of them as stored zeros in the oracle's level."""
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    for kw in (dict(true_pmax_elmts=0), {}):
        kw = dict(kw, interp_type=INTERP_TABLE_OPERATORS[name][2])
        plus, minus = device_setup(mi, name, kw), device_setup(mi, name, kw, sign=-1)
        assert plus.interp_census(0)["cap1024"] >= 4 and minus.interp_census(0) == plus.interp_census(0)
        zeros = []
        assert_mirrored_hierarchies(plus, minus, exact_zeros=zeros)
        oamg = oc.Amg(oc.Csr.from_scipy(operator(name)), oracle_params(oc, name, kw, gs_chunk=_chunk(mi)))
        print(name, kw, "entries that are exactly zero, per level:", zeros)
        assert zeros == [int((oamg.level_A(l).arrays()[2] == 0.0).sum()) for l in range(oamg.num_levels)]
        if "true_pmax_elmts" not in kw:
            assert sum(zeros) == 0  # (the truncated hierarchy mirrors without exception)


@pytest.mark.parametrize("name", ["overflow", "overflow_ext"])
def test_one_row_over_the_largest_table_falls_back_for_that_level_only(mi, oc, name, monkeypatch):
    """level 0 goes to the host routine, level 1 is the device's again; the hierarchy equals the oracle's bit for bit
    and GMRES(30) + AMG takes the oracle's iterations"""
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    M = operator(name)
    n = M.shape[0]
    kw = dict(interp_type=INTERP_TABLE_OPERATORS[name][2])
    A = mi.matrix_from_scipy(M)
    bv = M @ np.random.default_rng(5).standard_normal(n)
    b, x = mi.IJVector(0, n - 1, bv), mi.IJVector(0, n - 1, np.zeros(n))
    amg = mi.BoomerAMG(print_level=0, **library_kw(name, kw))
    gm = mi.GMRES(tolerance=1e-8, max_iterations=60, kspace=30, print_level=0)
    gm.set_precond(amg)
    gm.setup(A, b, x)
    rc = gm.solve(A, b, x)
    Ao = oc.Csr.from_scipy(M)
    oamg = oc.Amg(Ao, oracle_params(oc, name, kw, gs_chunk=_chunk(mi)))
    assert amg.num_levels > 2
    c0 = check_census(amg, predicted_census(*bounds(oc, name, kw["interp_type"])))
    assert c0["fell_back"] and 1024 < c0["max_bound"] <= 1040
    c1 = amg.interp_census(1)
    assert not c1["fell_back"] and not c1["host"] and sum(c1[k] for k in CENSUS_KEYS) == amg.level_csr(1, 0)[3][0] > 0
    _assert_same_hierarchy(amg, oamg)
    xo, info = oc.gmres(Ao, bv, kdim=30, tol=1e-8, maxit=60, amg=oamg)
    assert rc == 0 and info["converged"] and gm.num_iterations == info["iters"], (gm.num_iterations, info["iters"])
    assert np.abs(x.get() - xo).max() <= 1e-7 * max(1.0, np.abs(xo).max())


def test_poisoned_allocations_leave_the_same_bits(mi, monkeypatch):
    """MI_HYPRE_POISON_ALLOC=1 in a fresh process (every device block is handed out full of 0xFF): rows that write
    fewer entries than their slack holds (the dense operator without truncation: slack for up to 599 candidates counted
    with multiplicity, at most 67 distinct ones written), counters and flags that nobody cleared -- the hierarchies keep
    their bits"""
    monkeypatch.setenv("MI_HYPRE_DEVICE_SETUP_MIN_ROWS", "0")
    jobs = {"hubs:0:0": ("hubs", dict(interp_type=0, true_pmax_elmts=0)),
            "dense1600:6:0": ("dense1600", dict(interp_type=6, true_pmax_elmts=0))}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MI_HYPRE_POISON_ALLOC="1")
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "interp_tables_worker.py"), *jobs], env=env, cwd=root,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    got = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    for job, (name, kw) in jobs.items():
        amg = device_setup(mi, name, kw)
        assert got[job]["census"] == amg.interp_census(0) and got[job]["census"]["cap512"] >= 4
        assert got[job]["digest"] == hierarchy_digest(amg), job
