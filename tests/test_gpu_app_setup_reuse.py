"""hypre_app with `boomeramg_settings: mi_setup_reuse: 1` on the deck of tests/test_gpu_app_update_steps.py: the Setup of
every update step refreshes the hierarchy (one rank) or rebuilds it and says why (two ranks).  The steps scale A, so the
kept interpolation stays the one a fresh Setup would build: every step takes the iterations of the first solve, within
one, and ends at x = 1."""
import re

import pytest

from tests.test_gpu_app import _run, _run_ranks
from tests.test_gpu_app_update_steps import DECK

pytestmark = pytest.mark.gpu

REUSE_DECK = DECK + "  mi_setup_reuse: 1\n"


def _check(out, verdict):
    solves = re.findall(r"^Solve (\d+) : (\d+) iterations, final relative residual ([0-9.eE+-]+)", out, re.M)
    assert [int(s[0]) for s in solves] == [0, 1, 2], out[-3000:]
    iters = [int(s[1]) for s in solves]
    print("iterations per solve:", iters)
    assert all(abs(i - iters[0]) <= 1 for i in iters) and 2 < iters[0] < 40
    errs = [float(e) for e in re.findall(r"max \|x - 1\| = ([0-9.eE+-]+)", out)]
    assert len(errs) >= 3 and max(errs) < 1e-6, out[-3000:]
    setups = re.findall(r"^Setup (\d+) : AMG hierarchy (refreshed|rebuilt \(([^)]*)\)), ([0-9.]+) s", out, re.M)
    assert [int(s[0]) for s in setups] == [1, 2], out[-3000:]
    assert all((s[1] if verdict == "refreshed" else s[2]) == verdict for s in setups), setups


def test_both_update_steps_refresh(tmp_path):
    _check(_run(tmp_path, REUSE_DECK.format(dev=1)), "refreshed")


def test_two_ranks_rebuild_and_say_why(tmp_path):
    """and the rebuilds are those of a run that never had the switch: every solve's iterations and residual"""
    out = _run_ranks(tmp_path, REUSE_DECK.format(dev=1), 2, 29953)
    _check(out, "more than one rank")
    plain = _run_ranks(tmp_path, DECK.format(dev=1), 2, 29955)
    solve = r"^Solve \d+ : \d+ iterations, final relative residual [0-9.eE+-]+"
    assert re.findall(solve, out, re.M) == re.findall(solve, plain, re.M) and len(re.findall(solve, out, re.M)) == 3
