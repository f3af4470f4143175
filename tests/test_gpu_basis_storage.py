"""Krylov basis storage (HYPRE_MI_SetKrylovBasisStorage) on the device.

1. the kernels' instantiations on float basis vectors against their double instantiations fed the same, float-rounded
   values: bit for bit; the rounding variant of the posting scaling kernel;
2. whole solves: mode 1 (float slots) equals mode 2 (fp64 vectors of rounded values) in iteration count, residual
   history, x and final relative residual, bit for bit;
3. mode 2 against the restatement tests/basis_storage_ref.py on the cases tests/basis_storage_cases.py qualifies;
4. mode 0 is untouched, BiCGSTAB and PCG ignore the setting;
5. the counters: the basis of a mode 1 solve is float vectors;
6. refusals;
7. nothing reads memory it has not written (a child process with every block handed out full of 0xFF);
8. the driver key and the sample deck."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import basis_storage_cases as bc
from tests import basis_storage_gpu_common as bg
from tests.test_gpu_mgs_block import ALL_PASSES, FEW_PASSES, _inputs
from tests.test_mgs_block_spec import B as NB

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the scalar tail, one workgroup, just over one grid stride of the capped grid (768 workgroups x 512)
SIZES = (1, 2, 3, 511, 513, 393216 + 3)
MASS_M = (1, 8, 9, 17)  # across MASS_NV = 8: one, two and three passes


def rd(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _vec(mi, v):
    return mi.IJVector(0, len(v) - 1, v)


# ------------------------------------------------------------------ 1. kernels
@pytest.mark.parametrize("n", SIZES)
def test_float_kernels_equal_double_kernels_on_rounded_values(mi, n):
    """k::mass_dot, k::mass_axpy, k::lin_comb (init on and off) and every pass shape of k::mgs_block_pass: the float
    instantiation on vectors converted to float against the double instantiation on rd(vectors)"""
    rng = np.random.default_rng(7000 + n % 1000)
    V = rng.standard_normal((max(MASS_M), n))
    wv = rng.standard_normal(n)
    raw, rounded = [_vec(mi, v) for v in V], [_vec(mi, rd(v)) for v in V]
    assert np.any(rd(V) != V)
    w0 = _vec(mi, wv)
    for m in MASS_M:
        coef = rng.standard_normal(m)
        f = mi.vector_kernel_op(mi.VEC_MASS_DOT, raw[:m], None, w0, f32=True)
        d = mi.vector_kernel_op(mi.VEC_MASS_DOT, rounded[:m], None, w0)
        assert f.tobytes() == d.tobytes(), ("mass_dot", n, m)
        for op, kw in ((mi.VEC_MASS_AXPY, dict(scale=-1.0)), (mi.VEC_MASS_AXPY, dict(scale=0.3)),
                       (mi.VEC_LIN_COMB, dict(init=True)), (mi.VEC_LIN_COMB, dict(init=False))):
            w1, w2 = _vec(mi, wv), _vec(mi, wv)
            mi.vector_kernel_op(op, raw[:m], coef, w1, f32=True, **kw)
            mi.vector_kernel_op(op, rounded[:m], coef, w2, **kw)
            assert w1.get().tobytes() == w2.get().tobytes(), (op, n, m, kw)
            assert w1.get().tobytes() != wv.tobytes() or n == 0
    c, gram = _inputs(rng)
    P, Q = (raw[:NB], rounded[:NB]), (raw[NB:2 * NB], rounded[NB:2 * NB])
    for mp, mn, last in (FEW_PASSES if n > 100000 else ALL_PASSES):
        w1, w2 = _vec(mi, wv), _vec(mi, wv)
        sf, hf, nf = mi.mgs_block_pass(P[0][:mp], Q[0][:mn], last, c, gram, w1, f32=True)
        sd, hd, nd = mi.mgs_block_pass(P[1][:mp], Q[1][:mn], last, c, gram, w2)
        tag = (n, mp, mn, last)
        assert sf.tobytes() == sd.tobytes() and hf.tobytes() == hd.tobytes() and nf == nd, tag
        assert w1.get().tobytes() == w2.get().tobytes(), tag


@pytest.mark.parametrize("n", SIZES)
def test_scaling_kernel_rounds_and_fills_the_float_slot(mi, n):
    """the posting scaling kernel's rounding variant: the fp64 vector is rd of what the plain kernel leaves, element by
    element (the product first, then the rounding), the float slot holds the same values, the posted doubles and the
    flag are the plain kernel's; a norm that is not positive leaves vector and slot alone but still posts"""
    rng = np.random.default_rng(7100 + n % 1000)
    wv = rng.standard_normal(n)
    slot0 = rd(rng.standard_normal(n))
    for count in (1, 9, 255):
        slots = rng.standard_normal(count)
        slots[0] = float(wv @ wv)
        w1, w2, xd = _vec(mi, wv), _vec(mi, wv), _vec(mi, slot0)
        posted1, flag1, seq1 = mi.vector_kernel_op(mi.VEC_SCALE_POST, [], slots, w1)
        posted2, flag2, seq2 = mi.vector_kernel_op(mi.VEC_SCALE_POST, [], slots, w2, xd=xd, f32=True)
        assert posted1.tobytes() == posted2.tobytes() == slots.tobytes() and flag1 == seq1 and flag2 == seq2 == seq1 + 1
        want = rd(w1.get())
        assert w2.get().tobytes() == want.tobytes(), ("fp64 vector", n, count)
        assert xd.get().tobytes() == want.tobytes(), ("float slot", n, count)
        for bad in (0.0, -1.0):
            slots[0] = bad
            before = w2.get()
            xd2 = _vec(mi, slot0)
            posted, flag, seq = mi.vector_kernel_op(mi.VEC_SCALE_POST, [], slots, w2, xd=xd2, f32=True)
            assert posted.tobytes() == slots.tobytes() and flag == seq
            assert w2.get().tobytes() == before.tobytes() and xd2.get().tobytes() == slot0.tobytes(), ("untouched", n, bad)


def test_the_float_hook_has_no_fused_dot(mi):
    w, v = _vec(mi, np.ones(5)), _vec(mi, np.ones(5))
    with pytest.raises(mi.HypreError, match="VectorKernelOpF32"):
        mi.vector_kernel_op(mi.VEC_AXPY_DOT, [v], [1.0], w, f32=True)
    mi.call("HYPRE_ClearAllErrors")


# ------------------------------------------------------------------ 2. mode 1 equals mode 2
@pytest.fixture(scope="module")
def systems(mi):
    return bg.Systems(mi)


@pytest.fixture(scope="module")
def mode1(systems):
    """every solve of the contract under mode 1, once"""
    return {s[0]: systems.run(s, 1) for s in bg.SOLVES}


def _same(a, b):
    return (a["code"] == b["code"] and a["iters"] == b["iters"] and a["hist"].tobytes() == b["hist"].tobytes()
            and a["x"].tobytes() == b["x"].tobytes() and np.float64(a["rel"]).tobytes() == np.float64(b["rel"]).tobytes())


@pytest.mark.parametrize("spec", bg.SOLVES, ids=lambda s: s[0])
def test_mode_1_equals_mode_2(mi, systems, mode1, spec):
    r1, r2 = mode1[spec[0]], systems.run(spec, 2)
    print(f"{spec[0]}: {r1['iters']} iterations under mode 1, {r2['iters']} under mode 2, final {r1['rel']:.3e}")
    assert r1["code"] == 0 and r1["iters"] > 3 and r1["rel"] <= spec[5]
    assert not np.isnan(r1["x"]).any()
    assert _same(r1, r2)
    if spec[0] == "gmres20_plain":
        assert r1["iters"] > 20  # restarted
    if spec[0] == "gmres40_amg":
        r0 = systems.run(spec, 0)
        print(f"  mode 0: {r0['iters']} iterations")
        assert r0["iters"] <= r1["iters"]


@pytest.mark.parametrize("sid", ["gmres5_amg", "gmres12_three_components"])
def test_mode_1_equals_mode_2_without_kept_directions(mi, systems, mode1, sid):
    """x += M^-1 sum_j y_j p_j: the linear combination reads the stored basis (k::lin_comb on float vectors), and the
    update costs one more cycle per restart cycle and component"""
    spec = bg.by_id(sid)
    ncomp = systems.get(spec[1])[1].shape[0]
    mi.set_gmres_keep_directions(False)
    try:
        c0 = mi.counter("precond_cycles")
        r1 = systems.run(spec, 1)
        cycles = mi.counter("precond_cycles") - c0
        r2 = systems.run(spec, 2)
    finally:
        mi.set_gmres_keep_directions(True)
    assert r1["code"] == 0 and r1["iters"] > 3 and _same(r1, r2)
    assert cycles >= (r1["iters"] + 1) * ncomp


def _child(ids, **env):
    e = dict(os.environ, **{k: str(v) for k, v in env.items()})
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "basis_storage_worker.py")] + ids,
                       env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_mode_1_equals_mode_2_in_natural_order(mode1):
    """MI_HYPRE_GMRES_PERMUTED=0 (read once per process): apply_precond's path, no kept directions, no hand-over"""
    got = _child(["gmres5_amg", "cogmres1_amg"], MI_HYPRE_GMRES_PERMUTED=0)
    for sid, (d1, d2, iters) in got.items():
        assert d1 == d2 and iters > 3, sid
        assert d1 != bg.digest(mode1[sid])  # another summation order: really the other path


# ------------------------------------------------------------------ 3. mode 2 against the restatement
_TAB = {}


def _tabulated_amg(mi, op):
    """the library's default BoomerAMG cycle as a dense map (one column per unit vector), as test_gpu_krylov_paths.py"""
    if op not in _TAB:
        A = mi.matrix_from_scipy(bc.operator(op))
        n = bc.operator(op).shape[0]
        amg = mi.BoomerAMG(print_level=0, max_iterations=1, tolerance=0.0)
        amg.setup(A)
        e, u = mi.IJVector(0, n - 1, np.zeros(n)), mi.IJVector(0, n - 1, np.zeros(n))
        Bm = np.empty((n, n))
        for j in range(n):
            idx = np.array([max(j - 1, 0), j], dtype=np.int64)
            mi.call("HYPRE_IJVectorSetValues", e.h, 2, idx, np.array([0.0, 1.0]))
            u.fill(0.0)
            amg.solve(A, e, u)
            Bm[:, j] = u.get()
        _TAB[op] = Bm
    return _TAB[op]


@pytest.mark.parametrize("cid", bc.QUALIFYING)
def test_mode_2_against_the_restatement(mi, cid):
    """equal iteration count, history within HISTORY_BAR ||r_0|| (measured: tests/basis_storage_cases.py), and the
    residual of the returned x, recomputed with scipy, within the tolerance"""
    case = bc.by_id(cid)
    A, Bv = bc.operator(case["op"]), bc.rhs(case)
    r = bc.reference(case, _tabulated_amg(mi, case["op"]) if case["amg"] else None)
    assert bc.margin(r) > bc.HISTORY_BAR  # qualifies with the device's own cycle too
    nc, n = Bv.shape
    kw = dict(tolerance=case["tol"], max_iterations=case["max_iter"], kspace=case["kdim"], print_level=0)
    s = (mi.GMRES(**kw) if case["solver"] == "gmres" else
         mi.FlexGMRES(**kw) if case["solver"] == "fgmres" else mi.COGMRES(cgs=case["cgs"], **kw))
    if case["amg"]:
        s.set_precond(mi.BoomerAMG(print_level=0))
    Am = mi.matrix_from_scipy(A)
    b = mi.IJVector(0, n - 1, Bv[0]) if nc == 1 else mi.IJVector(0, n - 1, Bv, ncomp=nc)
    x = mi.IJVector(0, n - 1, np.zeros(n)) if nc == 1 else mi.IJVector(0, n - 1, np.zeros((nc, n)), ncomp=nc)
    with bg.basis_storage(mi, 2):
        s.setup(Am, b, x)
        assert s.solve(Am, b, x) == 0
    hist = s.residual_history()
    dev = np.abs(hist - r["norms"]).max() / r["norms"][0] if len(hist) == len(r["norms"]) else np.inf
    print(f"{cid}: {s.num_iterations} iterations (restatement {r['iters']}), history deviation / ||r_0|| = {dev:.3e}, "
          f"bar {bc.HISTORY_BAR:.3e}")
    assert s.num_iterations == r["iters"]
    assert dev <= bc.HISTORY_BAR
    xs = x.get_all() if nc > 1 else x.get()[None, :]
    res = np.linalg.norm(np.concatenate([Bv[c] - A @ xs[c] for c in range(nc)])) / np.linalg.norm(Bv)
    print(f"  ||b - A x|| / ||b|| = {res:.3e}")
    assert res <= case["tol"]


# ------------------------------------------------------------------ 4. mode 0 is untouched
def test_one_object_under_modes_0_1_0(mi, systems, mode1):
    """the basis is reallocated when the mode changes between two solves on one solver object"""
    for sid in ("gmres5_amg", "gmres20_plain"):
        spec = bg.by_id(sid)
        fresh0 = systems.run(spec, 0)
        one = bg.make_solver(mi, spec)
        assert _same(systems.run(spec, 0, solver=one), fresh0)
        assert _same(systems.run(spec, 1, solver=one), mode1[sid])
        assert _same(systems.run(spec, 0, solver=one), fresh0)
        assert _same(systems.run(spec, 2, solver=one), mode1[sid])
        assert fresh0["hist"].tobytes() != mode1[sid]["hist"].tobytes()


@pytest.mark.parametrize("name", ["BiCGSTAB", "PCG"])
def test_other_solvers_ignore_the_setting(mi, systems, name):
    A, Bv = systems.get("lap14")
    n = Bv.shape[1]
    res = {}
    for mode in (0, 1):
        s = getattr(mi, name)(tolerance=1e-10, max_iterations=60, print_level=0)
        s.set_precond(mi.BoomerAMG(print_level=0))
        b, x = mi.IJVector(0, n - 1, Bv[0]), mi.IJVector(0, n - 1, np.zeros(n))
        with bg.basis_storage(mi, mode):
            s.setup(A, b, x)
            assert s.solve(A, b, x) == 0
        res[mode] = dict(code=0, iters=s.num_iterations, hist=s.residual_history(), x=x.get(), rel=s.final_rel_res)
    assert res[0]["iters"] > 3 and _same(res[0], res[1])


# ------------------------------------------------------------------ 5. storage is really fp32
def test_the_basis_of_a_mode_1_solve_is_float_vectors(mi, systems):
    spec = ("one_cycle", "lap14", "gmres", 50, 0, 1e-5, True, 60)  # m iterations in one cycle: p_0 .. p_m
    n = systems.get(spec[1])[1].shape[1]
    f0 = mi.counter("krylov_basis_fp32_vectors")
    r1 = systems.run(spec, 1)
    m = r1["iters"]
    assert 3 < m < 50
    assert mi.counter("krylov_basis_fp32_vectors") - f0 == m + 1
    assert mi.counter("krylov_basis_bytes") == 4 * n * (m + 1)
    r2 = systems.run(spec, 2)
    assert r2["iters"] == r1["iters"]
    assert mi.counter("krylov_basis_fp32_vectors") - f0 == m + 1
    assert mi.counter("krylov_basis_bytes") == 8 * n * (m + 1)


# ------------------------------------------------------------------ 6. refusals
def test_other_modes_are_refused(mi):
    mi.set_basis_storage(1)
    try:
        for bad in (-1, 3):
            assert mi.call("HYPRE_MI_SetKrylovBasisStorage", bad, allow=(mi.HYPRE_ERROR_ARG,)) == mi.HYPRE_ERROR_ARG
            assert mi.get_basis_storage() == 1
            mi.call("HYPRE_ClearAllErrors")
    finally:
        mi.set_basis_storage(0)
    assert mi.get_basis_storage() == 0


def test_two_ranks_refuse_the_mode_by_name(tmp_path):
    """hypre_app on two ranks sharing the test GPU (launched as tests/test_gpu_app.py::_run_ranks does) with
    mi_basis_storage: 1: Solve is refused with a message that names the setting, on every rank, before any collective;
    no iteration is made -- the solve never runs as mode 0 in silence"""
    etc = os.path.join(ROOT, "hypre-mini-app_amd", "etc")
    deck = re.sub(r"(n[xyz]): 64", r"\1: 12", open(os.path.join(etc, "laplace_3d_basis_fp32.yaml")).read())
    (tmp_path / "input.yaml").write_text(deck)
    env = dict(os.environ, MI_HYPRE_TRANSPORT="tcp", HSA_ENABLE_IPC_MODE_LEGACY="0", MI_HYPRE_HOST_THREADS="2")
    cmd = ["timeout", "-k", "10", "200", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", "29967", "--no-python",
           os.path.join(ROOT, "hypre-mini-app_amd", "hypre_app"), "input.yaml"]
    p = subprocess.run(cmd, cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode not in (124, 137), p.stdout[-3000:]
    assert len(re.findall(r"Krylov basis storage mode 1 \(HYPRE_MI_SetKrylovBasisStorage / MI_HYPRE_BASIS_STORAGE\) runs on "
                          r"one rank only", p.stdout)) >= 2, p.stdout[-3000:]
    solves = re.findall(r"^Solve 0 : (\d+) iterations", p.stdout, re.M)
    assert solves in ([], ["0"]), p.stdout[-3000:]


# ------------------------------------------------------------------ 7. nothing reads unwritten memory
def test_nothing_reads_memory_it_has_not_written(mode1):
    """GMRES(5) behind BoomerAMG under mode 1 with MI_HYPRE_POISON_ALLOC=1: the float slots and the two work vectors are
    written before they are read"""
    got = _child(["gmres5_amg"], MI_HYPRE_POISON_ALLOC=1)
    assert got["gmres5_amg"][0] == got["gmres5_amg"][1] == bg.digest(mode1["gmres5_amg"])


# ------------------------------------------------------------------ 8. driver
def test_driver_deck(tmp_path):
    """hypre_app on etc/laplace_3d_basis_fp32.yaml at 32^3: converges to x = 1 in the iterations of the default deck at
    that tolerance, give or take the iteration of a false convergence"""
    from tests.test_gpu_app import _run

    etc = os.path.join(ROOT, "hypre-mini-app_amd", "etc")
    deck = re.sub(r"(n[xyz]): 64", r"\1: 32", open(os.path.join(etc, "laplace_3d_basis_fp32.yaml")).read())
    assert "mi_basis_storage: 1" in deck and "tolerance: 1.0e-6" in deck
    plain = re.sub(r"(n[xyz]): 64", r"\1: 32", open(os.path.join(etc, "laplace_3d.yaml")).read())
    plain = plain.replace("tolerance: 1.0e-8", "tolerance: 1.0e-6")
    assert "tolerance: 1.0e-6" in plain and "mi_basis_storage" not in plain
    its = {}
    for name, text in (("fp32", deck), ("fp64", plain)):
        d = tmp_path / name
        d.mkdir()
        out = _run(d, text)
        m = re.search(r"^Solve 0 : (\d+) iterations, final relative residual ([0-9.eE+-]+)", out, re.M)
        assert m and float(m.group(2)) <= 1e-6, out[-3000:]
        e = re.search(r"max \|x - 1\| = ([0-9.eE+-]+)", out)
        assert e and float(e.group(1)) < 1e-4, out[-3000:]
        its[name] = int(m.group(1))
    print("iterations:", its)
    assert 2 < its["fp64"] <= its["fp32"] <= its["fp64"] + 1
    bad = tmp_path / "bad"
    bad.mkdir()
    (bad / "input.yaml").write_text(deck.replace("mi_basis_storage: 1", "mi_basis_storage: 3"))
    p = subprocess.run([os.path.join(ROOT, "hypre-mini-app_amd", "hypre_app"), "input.yaml"], cwd=bad, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode != 0 and "mi_basis_storage" in p.stdout, p.stdout[-2000:]
