"""hypre_app with `linear_system: mi_device_assembly: 1`: the driver hands the entries and the vector indices over in
device memory (the synthetic system from the device generator, a MatrixMarket system copied to the device by the
loader) and the library assembles on the device.  Iteration count and printed final residual are those of the default
run, which hands over host arrays."""
import re

import pytest

from tests.test_gpu_app import DEFAULT_AMG, _run, _system, _write_mm_matrix, _write_mm_vector

pytestmark = pytest.mark.gpu

SOLVER = """
solver_settings:
  method: gmres
  preconditioner: boomeramg
  tolerance: 1.0e-10
  max_iterations: 100
  kspace: 50
  print_level: 2
""" + DEFAULT_AMG


def _result(out):
    m = re.search(r"Solve 0 : (\d+) iterations, final relative residual ([0-9.eE+-]+)", out)
    assert m, out[-2000:]
    return int(m.group(1)), m.group(2)


def test_small_laplace_with_and_without_device_assembly(tmp_path):
    res = []
    for key in ("", "mi_device_assembly: 1", "mi_device_assembly: 0"):
        d = tmp_path / f"run{len(res)}"
        d.mkdir()
        out = _run(d, f"""
linear_system:
  type: laplace_3d
  nx: 16
  ny: 16
  nz: 16
  stencil: 7
  {key}
""" + SOLVER)
        m = re.search(r"max \|x - 1\| = ([0-9.eE+-]+)", out)
        assert m and float(m.group(1)) < 1e-7, out[-2000:]
        on_device = "mi_device_assembly: 1 matrix assembled on the device, 0 entries fetched to the host" in out
        assert on_device == key.endswith("1"), out[-2000:]
        res.append(_result(out))
    assert res[0] == res[1] == res[2] and 2 < res[0][0] < 40


def test_matrix_market_loader_with_device_assembly(tmp_path):
    A, b, x = _system(24, 3, nonsym=True)
    res = []
    for key in ("", "mi_device_assembly: 1"):
        d = tmp_path / f"run{len(res)}"
        d.mkdir()
        _write_mm_matrix(d / "mat.mm", A)
        _write_mm_vector(d / "rhs.mm", b)
        _write_mm_vector(d / "sln.mm", x)
        out = _run(d, f"""
linear_system:
  type: matrix_market
  matrix_file: mat.mm
  rhs_file: rhs.mm
  sln_file: sln.mm
  rtol: 1.0e-5
  atol: 1.0e-7
  {key}
""" + SOLVER)
        assert "allClose=1" in out
        on_device = "mi_device_assembly: 1 matrix assembled on the device, 0 entries fetched to the host" in out
        assert on_device == bool(key), out[-2000:]
        res.append(_result(out))
    assert res[0] == res[1]
