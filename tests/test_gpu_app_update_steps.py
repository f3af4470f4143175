"""hypre_app with `linear_system: mi_update_steps: K`: after the first solve the driver gives its IJ matrix new values in
place K times (Initialize, SetConstantValues(0), the same entries scaled by 1 + 0.5 * step added, Assemble), scales the
right-hand side alike, sets preconditioner and solver up again and solves.  A scaled operator gives the same hierarchy up
to scaling, so every step takes the iterations of the first solve and ends at x = 1."""
import re

import pytest

from tests.test_gpu_app import DEFAULT_AMG, _run, _run_ranks

pytestmark = pytest.mark.gpu

DECK = """
linear_system:
  type: laplace_3d
  nx: 16
  ny: 16
  nz: 16
  stencil: 7
  mi_update_steps: 2
  mi_device_assembly: {dev}

solver_settings:
  method: gmres
  preconditioner: boomeramg
  tolerance: 1.0e-10
  max_iterations: 100
  kspace: 50
  print_level: 2
""" + DEFAULT_AMG


def _check(out):
    solves = re.findall(r"^Solve (\d+) : (\d+) iterations, final relative residual ([0-9.eE+-]+)", out, re.M)
    assert [int(s[0]) for s in solves] == [0, 1, 2], out[-3000:]
    errs = [float(e) for e in re.findall(r"max \|x - 1\| = ([0-9.eE+-]+)", out)]
    assert len(errs) >= 3 and max(errs) < 1e-6, out[-3000:]
    iters = [int(s[1]) for s in solves]
    print("iterations per solve:", iters)
    assert max(iters) - min(iters) <= 1 and 2 < iters[0] < 40
    assert out.count("Update step") == 2
    return iters


@pytest.mark.parametrize("dev", [1, 0])
def test_two_update_steps(tmp_path, dev):
    _check(_run(tmp_path, DECK.format(dev=dev)))


def test_two_update_steps_on_two_ranks(tmp_path):
    _check(_run_ranks(tmp_path, DECK.format(dev=1), 2, 29951))
