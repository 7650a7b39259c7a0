"""CPU tests of the post-training evaluation surface (cnf_ot_amd.applications / solvers): the closed forms, the
command line, and the argument checks that come before any device work."""
import math
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rwpo_true_value_quadratic_and_ou_variance_closed_forms():
  from cnf_ot_amd import applications as app
  for dim, T, beta in ((2, 1, 1), (2, 2, 10), (10, 1.5, 4.0)):
    assert app.rwpo_true_value(dim, T, beta, 1.0, "quadratic") == pytest.approx(dim * (1 + math.log(T + 1)) / beta,
                                                                               rel=1e-15)
  assert app.rwpo_true_value(2, 1, 1, 0.0, "quadratic") == pytest.approx(3.3863, abs=5e-5)
  assert app.rwpo_true_value(2, 1, 1, 0.0, "obstacle") is None
  for t, a, v0, s in ((1.0, 1.0, 4.0, 0.5), (0.3, 2.0, 1.0, 0.5), (2.0, 0.5, 1.5, 1.0), (0.0, 1.0, 3.0, 0.25)):
    assert app.ou_variance(t, a, v0, s) == pytest.approx(math.exp(-2 * a * t) * (v0 - s / a) + s / a, rel=1e-15)
  # sigma = 1/2 is the reference's target variance (solvers.py:246-252: exp(-2 a T) (4 - 1/2/a) + 1/2/a)
  assert app.ou_variance(1.0, 1.0, 4.0) == pytest.approx(math.exp(-2.0) * 3.5 + 0.5, rel=1e-15)
  assert app.ou_variance(0.0, 1.0, 4.0) == 4.0


def test_solvers_command_line_help_lists_its_flags():
  r = subprocess.run([sys.executable, "-m", "cnf_ot_amd.solvers", "--help"], cwd=ROOT, capture_output=True, text=True,
                     timeout=120)
  assert r.returncode == 0, r.stderr
  for flag in ("--config", "--epochs", "--capture", "--save"):
    assert flag in r.stdout


def test_evaluation_argument_checks_need_no_device():
  from cnf_ot_amd import FlowConfig, FlowModel, applications as app
  model = FlowModel(FlowConfig(dim=3))
  with pytest.raises(ValueError):
    app.density_l2_grid_error_fn(model, 1.0, 1.0, None, 1.0)
  with pytest.raises(ValueError):
    app.rwpo_true_value(dim=3, T=1.0, beta=1.0, a=1.0, subtype="double_well")
  with pytest.raises(ValueError):
    app.rwpo_true_value(dim=2, T=1.0, beta=1.0, a=1.0, subtype="no_such_potential")
