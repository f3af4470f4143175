"""bench.py --dump-outputs without a device: which rows of the solution are written, how, and within what size."""
import importlib.util
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_output_rows_all_or_fixed_sample():
    b = _bench()
    assert np.array_equal(b.output_rows(1000), np.arange(1000))
    n = 512 ** 3
    r = b.output_rows(n)
    assert r.dtype == np.int64 and 0.95 * b.DUMP_MAX_VALUES < r.size <= b.DUMP_MAX_VALUES
    assert r[0] >= 0 and r[-1] < n and np.all(np.diff(r) > 0)
    assert np.array_equal(r, b.output_rows(n))  # the same rows in every run
    assert b.output_rows(n, 3).size <= b.DUMP_MAX_VALUES // 3


def test_dump_outputs_writes_float64_within_bound(tmp_path):
    b = _bench()
    n = b.DUMP_MAX_VALUES + 300000  # sampled: more rows than DUMP_MAX_VALUES
    xs = np.arange(n, dtype=np.float64)[None, :]  # x[i] = i: the file names the rows it holds
    b.dump_outputs(str(tmp_path), None, 0, 0, xs, n, {"iterations": 17, "final_rel_residual": 1e-9})
    x = np.load(tmp_path / "x.npy")
    assert x.dtype == np.float64 and np.array_equal(x, b.output_rows(n).astype(np.float64))
    assert np.load(tmp_path / "iterations.npy").tolist() == [17.0]
    assert np.load(tmp_path / "final_rel_residual.npy").dtype == np.float64
    assert sum(f.stat().st_size for f in tmp_path.iterdir()) <= 64 << 20


def test_steps_must_be_positive():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 2 and "--steps" in p.stdout, p.stdout[-2000:]
