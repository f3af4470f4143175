"""CPU: unknown-based systems AMG (HYPRE_BoomerAMGSetNumFunctions / SetDofFunc; DESIGN.md section 3, "Systems of PDEs")
through HYPRE_MI_BoomerAMGSetupHostOnly, against the level-by-level restatement in tests/systems_ref.py: cf and P of
every level are those of a scalar two-level setup on the numpy-filtered operator (P bit for bit), the coarse operator is
the triple product with the FULL A, dof_func follows the C points, P links equal functions only.  Then the refusals,
the reuse verdict, num_functions 1 and the host filter routine."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from tests import systems_cases as sc
from tests import systems_ref as ref
from tests.agg2s_common import ROOT, ij_host

_cache = {}


def system(name):
    if name not in _cache:
        _cache[name] = sc.case(name)
    return _cache[name]


def host_setup(mi, M, **kw):
    amg = mi.BoomerAMG(print_level=0, **kw)
    A = ij_host(mi, M)
    mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
    amg.keep_matrix = A
    return amg


def test_symbols_declared_and_exported(mi_lib):
    strip = lambda p: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", p)).read(), flags=re.S)
    ls, ext = strip("HYPRE_parcsr_ls.h"), strip("HYPRE_mi_ext.h")
    for name in ("HYPRE_BoomerAMGSetNumFunctions", "HYPRE_BoomerAMGGetNumFunctions", "HYPRE_BoomerAMGSetDofFunc"):
        assert re.search(r"HYPRE_Int\s+%s\s*\(" % name, ls) and hasattr(mi_lib.lib(), name), name
    for name in ("HYPRE_MI_BoomerAMGGetLevelDofFunc", "HYPRE_MI_SameFunctionFilterOp"):
        assert re.search(r"HYPRE_Int\s+%s\s*\(" % name, ext) and hasattr(mi_lib.lib(), name), name
    amg = mi_lib.BoomerAMG(print_level=0)
    assert amg.num_functions == 1
    assert mi_lib.BoomerAMG(print_level=0, num_functions=3).num_functions == 3


def test_cases_are_what_they_claim():
    M, dof, k, _ = system("lame1")
    assert M.shape == (3 * 729, 3 * 729) and abs(M - M.T).max() == 0.0 and np.diff(M.indptr).max() == 15
    assert k == 3 and np.array_equal(dof, np.arange(M.shape[0]) % 3)
    Mm, dm, _, _ = system("lame1_major")
    old = (np.arange(M.shape[0]) % 3) * 729 + np.arange(M.shape[0]) // 3
    assert abs(Mm[old][:, old] - M).max() == 0.0 and np.array_equal(dm[old], dof)
    for name in sc.CASES:
        M, dof, k, default = system(name)
        assert abs(M - M.T).max() <= 1e-15 and (M.diagonal() > 0).all()
        assert set(np.unique(dof)) == set(range(k))
        assert default == np.array_equal(dof, np.arange(M.shape[0]) % k)
        F = ref.filter_same_function(M, dof)
        assert 0 < F.nnz < M.nnz  # there is something to filter


# every case under the default interpolation, every setting on the Lame and the 3-field case
PAIRS = [(name, "interp6") for name in sc.CASES] + \
        [(name, s) for name in ("lame10", "diff3") for s in sc.SETTINGS if s != "interp6"] + \
        [("diff3_random", "interp17"), ("lame1_major", "agg5")]


@pytest.mark.parametrize("name,setting", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_every_level_is_the_scalar_setup_of_the_same_function_operator(mi_lib, oc, name, setting):
    mi = mi_lib
    M, dof, k, default = system(name)
    kw = sc.amg_kwargs(setting, k, dof, default)
    amg = host_setup(mi, M, **kw)
    assert amg.num_levels >= 3, amg.num_levels
    checked = ref.check_hierarchy(mi, oc, amg, M, dof, kw)
    assert checked == amg.num_levels - 1


def test_the_unknown_approach_is_not_the_scalar_hierarchy(mi_lib):
    """the feature does something.  On the Lame case the mixed derivatives are weak on level 0: both setups make the
    same splitting and the same pattern of P there, with other weights (the scalar setup lumps the mixed derivatives
    into the diagonal, the unknown approach leaves them out); from level 1 on the scalar setup's splitting differs and
    its P mixes the displacement components"""
    mi = mi_lib
    M, dof, k, _ = system("lame10")
    kw = dict(sc.SETTINGS["interp6"], strong_threshold=sc.THETA)
    a1, a3 = host_setup(mi, M, **kw), host_setup(mi, M, num_functions=3, **kw)
    l1, l3 = ref.product_levels(a1, with_dof=False), ref.product_levels(a3)
    assert np.array_equal(l1[0]["cf"], l3[0]["cf"])
    assert np.array_equal(l1[0]["P"].indices, l3[0]["P"].indices) and abs(l1[0]["P"] - l3[0]["P"]).max() > 1e-3
    assert not np.array_equal(l1[1]["cf"], l3[1]["cf"])
    P = sp.coo_matrix(l1[1]["P"])
    d1 = ref.coarse_dof_func(dof, l1[0]["cf"])
    assert (d1[P.row] != ref.coarse_dof_func(d1, l1[1]["cf"])[P.col]).sum() > 100


@pytest.mark.parametrize("setting", ["interp6", "agg5"])
def test_num_functions_1_is_bit_identical_to_no_call_at_all(mi_lib, setting):
    mi = mi_lib
    M, dof, k, _ = system("diff3_random")
    kw = dict(sc.SETTINGS[setting], strong_threshold=sc.THETA)
    base = host_setup(mi, M, **kw)
    for extra in (dict(num_functions=1), dict(num_functions=1, dof_func=dof)):
        amg = host_setup(mi, M, **kw, **extra)
        assert amg.num_levels == base.num_levels >= 3
        for l in range(base.num_levels):
            for which in (0, 2, 3) if l < base.num_levels - 1 else (0,):
                x, y = base.level_csr(l, which), amg.level_csr(l, which)
                assert all(np.array_equal(p, q) for p, q in zip(x[:3], y[:3])) and x[3] == y[3], (l, which)
            assert np.array_equal(base.level_perm(l), amg.level_perm(l))
            if l < base.num_levels - 1:
                assert np.array_equal(base.level_cf(l), amg.level_cf(l))
        with pytest.raises(mi.HypreError, match="built with num_functions 1"):
            amg.level_dof_func(0)
        mi.call("HYPRE_ClearAllErrors")


def refused(mi, M, pattern, **kw):
    amg = mi.BoomerAMG(print_level=0, **kw)
    A = ij_host(mi, M)
    with pytest.raises(mi.HypreError, match=pattern):
        mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
    mi.call("HYPRE_ClearAllErrors")


def test_refusals_by_name(mi_lib):
    mi = mi_lib
    M, dof, k, _ = system("diff2_weak")
    for bad in (0, -2):
        refused(mi, M, r"num_functions %d is not implemented \(a value >= 1 is\)" % bad, num_functions=bad)
    d = dof.copy()
    d[37] = 2
    refused(mi, M, r"dof_func\[37\] = 2 \(local row 37\) is outside \[0, num_functions = 2\)", num_functions=2, dof_func=d)
    d[37], d[5] = 0, -1
    refused(mi, M, r"dof_func\[5\] = -1 \(local row 5\) is outside", num_functions=2, dof_func=d)
    refused(mi, M, r"restriction 1 \(approximate ideal restriction\) with num_functions 2 is not implemented",
            num_functions=2, restriction=1)
    # the bad dof_func is not looked at while num_functions is 1
    assert host_setup(mi, M, num_functions=1, dof_func=d).num_levels >= 2


def test_more_than_one_rank_is_refused_for_the_distributed_and_the_replicated_setup():
    env = dict(os.environ, MI_HYPRE_HOST_THREADS="2", OMP_NUM_THREADS="1", MI_HYPRE_LOCALITY_ORDER="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", "30967", os.path.join(ROOT, "tests", "systems_dist_worker.py")]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    assert p.stdout.count("systems rank ok") == 2, p.stdout[-4000:]


def test_setup_reuse_rebuilds_with_reason_4(mi_lib):
    mi = mi_lib
    M, dof, k, _ = system("diff2_weak")
    amg = mi.BoomerAMG(print_level=0, num_functions=2, setup_reuse=1, strong_threshold=sc.THETA)
    A = ij_host(mi, M)
    mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
    assert amg.setup_kind() == (1, 1)
    mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
    assert amg.setup_kind() == (1, 4)
    mi.lib().HYPRE_MI_SetupReuseReasonText.restype = mi.C.c_char_p
    assert b"num_functions > 1" in mi.lib().HYPRE_MI_SetupReuseReasonText(4)
    ext = open(os.path.join(ROOT, "include", "HYPRE_mi_ext.h")).read()
    assert re.search(r"4 a setting the refresh does not cover[^;]*num_functions > 1", ext, re.S)
    # num_functions is a structural setting: back to 1 the kept hierarchy is not refreshed but rebuilt, then kept
    mi.call("HYPRE_BoomerAMGSetNumFunctions", amg.h, 1)
    mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
    assert amg.setup_kind() == (1, 3)
    mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", amg.h, A.par)
    assert amg.setup_kind() == (2, 0)


def ragged_matrix(n, seed, diag_every=3):
    """rows of 0 ... 40 entries, every diag_every-th row without a stored diagonal"""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for i in range(n):
        c = set(int(j) for j in rng.choice(n, size=min(n, int(rng.integers(0, 41))), replace=False))
        c.discard(i)
        if i % diag_every:
            c.add(i)
        rows += [i] * len(c)
        cols += sorted(c)
    M = sp.csr_matrix((rng.standard_normal(len(rows)), (rows, cols)), shape=(n, n))
    M.sort_indices()
    return M


@pytest.mark.parametrize("k", [1, 2, 3, 7])
def test_host_filter_routine_against_numpy_bitwise(mi_lib, k):
    mi = mi_lib
    M = ragged_matrix(300, seed=k)
    dof = np.random.default_rng(100 + k).integers(0, k, size=300).astype(np.int32)
    ia, ja, a, shape = mi.same_function_filter_op(M, dof, host=True)
    F = ref.filter_same_function(M, dof)
    assert np.array_equal(ia, F.indptr) and np.array_equal(ja, F.indices) and np.array_equal(a, F.data)
    assert (k > 1) == (F.nnz < M.nnz)
    for name in ("lame1", "diff3_random"):
        Ms, ds, _, _ = system(name)
        ia, ja, a, _ = mi.same_function_filter_op(Ms, ds, host=True)
        F = ref.filter_same_function(Ms, ds)
        assert np.array_equal(ia, F.indptr) and np.array_equal(ja, F.indices) and np.array_equal(a, F.data)
