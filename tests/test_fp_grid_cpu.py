"""The finite-volume Fokker-Planck reference's float64 restatement (tests/fp_grid_f64.py) against closed forms, and the
refusals of applications.fp_reference_grid that need no device.  No GPU.

The bounds on the L1 errors are the scheme's own measured errors (ou: 1.63e-3 at 65 points per axis and 3.0e-4 at 129,
ratio 5.4; nongradient: 2.50e-3 and 5.1e-4) with headroom below a factor 1.6; the step counts are exact."""
import math

import numpy as np
import pytest

import fp_grid_f64 as fg
from cnf_ot_amd import applications as app

BOX = (-6.0, 6.0, -6.0, 6.0)
A, SIGMA, T, VAR0 = 1.0, 0.5, 1.0, 1.0
_CACHE = {}


def solved(subtype, n, box=BOX):
  key = (subtype, n, box)
  if key not in _CACHE:
    _CACHE[key] = fg.solve(box, n, A, SIGMA, subtype, [T], var0=VAR0)
  return _CACHE[key]


def l1_error(subtype, n):
  r = solved(subtype, n)
  _, _, dx, dy = fg.axes_of(BOX, n)
  exact = fg.gaussian_at_centres(BOX, n, app.ou_variance(T, A, VAR0, SIGMA))
  return float(np.abs(r["density"][0] - exact).sum() * dx * dy)


def test_ou_converges_to_the_exact_gaussian():
  e65, e129 = l1_error("ou", 65), l1_error("ou", 129)
  print("ou L1", e65, e129, e65 / e129)
  assert e65 < 2.5e-3
  assert e129 < 5e-4
  assert e65 / e129 > 4.0


def test_ou_variance():
  _, cov = fg.moments(solved("ou", 129)["stats"][0])
  exact = app.ou_variance(T, A, VAR0, SIGMA)
  print("ou variance", cov[0, 0], cov[1, 1], exact)
  assert abs(cov[0, 0] - exact) < 4e-4 and abs(cov[1, 1] - exact) < 4e-4


def test_nongradient_keeps_the_isotropic_gaussian():
  e65, e129 = l1_error("nongradient", 65), l1_error("nongradient", 129)
  print("nongradient L1", e65, e129)
  assert e65 < 3.5e-3
  assert e129 < 7e-4
  for n in (65, 129):
    _, cov = fg.moments(solved("nongradient", n)["stats"][0])
    assert abs(cov[0, 1]) < 1e-12


@pytest.mark.parametrize("subtype,box", [("ou", BOX), ("nongradient", BOX), ("smile", (-4.0, 4.0, -4.0, 4.0))])
def test_positive_and_conservative(subtype, box):
  r = solved(subtype, 65, box)
  _, _, dx, dy = fg.axes_of(box, 65)
  mass0 = fg.initial(box, 65, VAR0).sum() * dx * dy
  assert r["density"].min() >= 0.0
  assert abs(r["stats"][0, 0] - mass0) <= 1e-13


def test_step_counts():
  assert int(solved("ou", 65)["n_steps"][0]) == 86
  assert int(solved("ou", 129)["n_steps"][0]) == 278
  assert int(solved("nongradient", 65)["n_steps"][0]) == 90
  assert int(solved("smile", 65, (-4.0, 4.0, -4.0, 4.0))["n_steps"][0]) == 2014


def test_helpers_agree_with_the_restatement():
  g = app.stats_grid((BOX, (9, 7)), (0, 1), 2)
  assert np.array_equal(app.fp_grid_initial(g, 0.7), fg.initial(BOX, (9, 7), 0.7))
  for delta, R in ((0.0, 77.0), (1.0, 77.4), (0.3, 1e-3), (0.9, 10.0)):
    assert app.fp_grid_step_count(delta, R) == fg.step_count(delta, R)


GRID = (BOX, 9)


@pytest.mark.parametrize("kwargs", [
  dict(subtype="no_such_drift"),
  dict(subtype="lorenz"),
  dict(sigma=0.0),
  dict(sigma=-1.0),
  dict(safety=0.0),
  dict(safety=1.5),
  dict(times=[-0.1, 0.5]),
  dict(times=[0.5, 0.5]),
  dict(times=[0.5, 0.2]),
  dict(times=[]),
  dict(times=list(np.linspace(0.0, 1.0, app.FP_MAX_SNAPSHOTS + 1))),
  dict(rho0=np.ones((9, 8))),
  dict(rho0=-np.ones((9, 9))),
  dict(steps_per_launch=3),
  dict(steps_per_launch=16),
])
def test_refusals_need_no_device(kwargs, monkeypatch):
  import torch

  def no_device(*a, **k):
    raise AssertionError("device work before the refusal")

  monkeypatch.setattr(torch.cuda, "current_device", no_device)
  args = dict(T=1.0, a=1.0, sigma=0.5, subtype="ou", times=[0.5, 1.0], grid=GRID)
  args.update(kwargs)
  with pytest.raises(ValueError):
    app.fp_reference_grid(**args)
