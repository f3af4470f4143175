"""One configuration of unknown-based systems AMG on the device, in a process of its own (the switches it runs under --
MI_HYPRE_DEVICE_SETUP_MIN_ROWS, MI_HYPRE_LOCALITY_ORDER, MI_HYPRE_POISON_ALLOC -- are the parent's to set):
tests/test_gpu_systems_amg.py.

    systems_worker.py hierarchy CASE SETTING    the device hierarchy against the host-only one, bit for bit: A, P, R,
                                                cf, the permutation and dof_func of every level
    systems_worker.py locality CASE             with the internal numbering: level 0's dof_func through its permutation
                                                is the caller's, and GMRES + AMG converges

Prints "RESULT <json>" with a digest of the device hierarchy, so that two runs can be compared."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from tests import systems_cases as sc  # noqa: E402
from tests.agg2s_common import ij_host  # noqa: E402


def device_matrix(mi, M):
    A = mi.IJMatrix(0, M.shape[0] - 1)
    coo = M.tocoo()
    A.set_values_coo(coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data.astype(np.float64))
    A.assemble()
    return A


def level_arrays(amg, l, last):
    out = []
    for which in (0,) if last else (0, 2, 3):
        ia, ja, a, shape = amg.level_csr(l, which)
        out += [np.asarray(shape, dtype=np.int64), ia, ja, a]
    out.append(amg.level_perm(l))
    out.append(amg.level_dof_func(l))
    if not last:
        out.append(amg.level_cf(l))
    return out


def compare_and_digest(dev, host):
    assert dev.num_levels == host.num_levels >= 3, (dev.num_levels, host.num_levels)
    h = hashlib.sha256()
    for l in range(dev.num_levels):
        last = l == dev.num_levels - 1
        for q, (x, y) in enumerate(zip(level_arrays(dev, l, last), level_arrays(host, l, last))):
            assert x.dtype == y.dtype and np.array_equal(x, y), "level %d, array %d differs from the host-only setup" % (l, q)
            h.update(np.ascontiguousarray(x).tobytes())
    return h.hexdigest()


def hierarchy(mi, case, setting):
    M, dof, k, default = sc.case(case)
    kw = sc.amg_kwargs(setting, k, dof, default)
    A, Ah = device_matrix(mi, M), ij_host(mi, M)
    dev = mi.BoomerAMG(print_level=0, **kw)
    dev.setup(A)
    host = mi.BoomerAMG(print_level=0, **kw)
    mi.call("HYPRE_MI_BoomerAMGSetupHostOnly", host.h, Ah.par)
    digest = compare_and_digest(dev, host)
    # the device built the levels: interp_type 6 / 0 by sk::interp, nothing handed to a host routine
    census = [dev.interp_census(l) for l in range(dev.num_levels - 1)]
    if kw.get("interp_type") in (0, 6) and not kw.get("agg_num_levels"):
        assert all(not c["host"] and not c["fell_back"] for c in census), census
    return dict(levels=dev.num_levels, digest=digest, rows=[int(dev.level_csr(l, 0)[3][0]) for l in range(dev.num_levels)])


def locality(mi, case):
    M, dof, k, default = sc.case(case)
    kw = sc.amg_kwargs("interp6", k, dof, default)
    A = device_matrix(mi, M)
    amg = mi.BoomerAMG(print_level=0, **kw)
    b = mi.IJVector(0, M.shape[0] - 1, M @ np.ones(M.shape[0]))
    x = mi.IJVector(0, M.shape[0] - 1, np.zeros(M.shape[0]))
    gm = mi.GMRES(tolerance=1e-8, max_iterations=60, kspace=60, print_level=0)
    gm.set_precond(amg)
    gm.setup(A, b, x)
    applied, order = amg.input_ordering()
    assert applied and not np.array_equal(order, np.arange(len(order)))
    # level 0's rows -> caller rows: GetLevelPerm(0) already holds the internal numbering; taken apart, the C-first
    # permutation of the internally numbered level composed with the input ordering is the same map
    perm0 = amg.level_perm(0)
    assert np.array_equal(np.sort(perm0), np.arange(len(perm0)))
    pos = np.empty(len(order), dtype=np.int64)
    pos[order] = np.arange(len(order))
    inner = pos[perm0]  # the C-first permutation alone (rows of the internal numbering)
    assert np.array_equal(order[inner], perm0)
    back = np.empty(len(perm0), dtype=np.int64)
    back[perm0] = amg.level_dof_func(0)
    assert np.array_equal(back, dof), "GetLevelDofFunc(0) through GetLevelPerm(0) is not the caller's dof_func"
    for l in range(amg.num_levels - 1):  # and on every level dof_func follows the C points
        d, cf, permc = amg.level_dof_func(l), amg.level_cf(l), amg.level_perm(l + 1)
        assert np.array_equal(d[cf == 1][permc], amg.level_dof_func(l + 1)), l
    rc = gm.solve(A, b, x)
    assert rc == 0 and gm.final_rel_res <= 1e-8, (rc, gm.final_rel_res)
    assert np.abs(x.get() - 1.0).max() < 1e-5
    return dict(levels=amg.num_levels, iters=gm.num_iterations)


def main():
    mi = ge.load_binding()
    mi.init()
    if sys.argv[1] == "hierarchy":
        out = hierarchy(mi, sys.argv[2], sys.argv[3])
    else:
        out = locality(mi, sys.argv[2])
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
