"""CPU tests of the fp particle reference: the host-side argument checks of cnf_fp_particles / cnf_point_stats through the
C ABI (no device is touched), the Python entry points' refusals, and the float64 restatement (tests/fp_particles_f64.py)
that the GPU tests hold the kernels to -- pinned against the Euler-Maruyama moment recursion for the Ornstein-Uhlenbeck
drift and against a plain explicit-Euler loop for Lorenz without noise.

Ornstein-Uhlenbeck bounds (N = 65 536 particles, per-dimension variance v of the scheme's own recursion
v <- (1 - a h)^2 v + 2 sigma h, exact for Euler-Maruyama where the continuous ou_variance is not): five standard errors
of each Gaussian sample statistic -- variance 5 v sqrt(2 / (N - 1)), mean 5 sqrt(v / N), off-diagonal covariance
5 v / sqrt(N).  OU_SEED is fixed where the restatement sits within three of them, so the GPU run, whose float32 normals
differ from the oracle's float64 evaluation in the last bits only, has margin.
"""
import math

import numpy as np
import pytest

import fp_particles_f64 as fp

OU, OU_SEED, ou_check = fp.OU, fp.OU_SEED, fp.ou_check


def test_ou_statistics_of_the_restatement(oracle_lib):
  from oracle import capi
  N, D, n = OU["N"], OU["D"], OU["n_steps"]
  R = fp.stream_stride(n, D)
  assert R == 204 and R % 4 == 0 and R >= (n + 1) * D
  z = fp.particle_normals(capi.normal(OU_SEED, 0, N * R), N, n, D)
  pos = fp.integrate(z, "ou", OU["a"], OU["sigma"], OU["h"], OU["var0"], OU["snaps"])
  assert pos.shape == (3, N, D)
  count, mean, cov = fp.moments(fp.stats(pos)[0], D)
  assert ou_check(count, mean, cov, f"restatement seed {OU_SEED}") <= 3.0      # the margin OU_SEED was chosen for
  # the recursion itself: the matrix form reduces to the scalar one, and both tend to the continuous closed form
  m, C = fp.em_moments(fp.linear_drift_matrix("ou", OU["a"], D), np.zeros(D), OU["var0"] * np.eye(D), OU["sigma"],
                       OU["h"], 100)
  v = fp.em_ou_variance(OU["var0"], OU["a"], OU["sigma"], OU["h"], 100)
  assert np.abs(C - v * np.eye(D)).max() <= 1e-15 and not m.any()
  fine = fp.em_ou_variance(2.0, 1.0, 0.5, 1e-5, 100000)
  exact = math.exp(-2.0) * (2.0 - 0.5) + 0.5
  assert abs(fine - exact) <= 1e-5


def test_stream_layout_and_start():
  flat = np.arange(3 * 16, dtype=np.float64)             # D = 3, 4 steps: 15 elements per particle, R = 16
  assert fp.stream_stride(4, 3) == 16
  z = fp.particle_normals(flat, 3, 4, 3)
  assert z.shape == (3, 5, 3) and z[1, 0, 0] == 16 and z[1, 2, 1] == 16 + 7 and z[2, 4, 2] == 32 + 14
  x0 = np.full((3, 3), 2.5)
  a = fp.integrate(z, "ou", 1.0, 0.5, 0.1, 4.0, (0, 2))
  b = fp.integrate(z, "ou", 1.0, 0.5, 0.1, 4.0, (0, 2), x0=x0)
  assert np.array_equal(a[0], 2.0 * z[:, 0]) and np.array_equal(b[0], x0)
  # a given start does not move the steps' draws
  step = lambda x, k: (x + 0.1 * fp.drift(x, "ou", 1.0)) + math.sqrt(2 * 0.5 * 0.1) * z[:, k]
  assert np.array_equal(b[1], step(step(x0, 1), 2))


def test_lorenz_without_noise_is_explicit_euler():
  rng = np.random.default_rng(3)
  N, n, h = 50, 200, 0.005
  z = rng.standard_normal((N, n + 1, 3))
  got = fp.integrate(z, "lorenz", 1.0, 0.0, h, 1.7, (0, 1, 77, n))
  c289, c83 = float(np.float32(28.0) / np.float32(9.0)), float(np.float32(8.0) / np.float32(3.0))
  x = math.sqrt(1.7) * z[:, 0]
  want = {0: x.copy()}
  for k in range(1, n + 1):
    X, Y, Z = x[:, 0], x[:, 1], x[:, 2]
    d = np.stack([10.0 * (Y - X), 9.0 * X * (c289 - Z) - Y, 9.0 * X * Y - c83 * Z], 1)
    x = x + h * d
    want[k] = x.copy()
  for s, k in enumerate((0, 1, 77, n)):
    assert np.abs(got[s] - want[k]).max() <= 1e-12 * max(1.0, np.abs(want[k]).max()), k
  assert np.isfinite(got).all() and np.abs(got[3] - got[0]).max() > 1.0       # the paths did move


def test_drifts_against_their_formulas():
  x = np.array([[0.3, -1.2, 2.0]])
  assert np.allclose(fp.drift(x[:, :2], "gradient", 2.0), 2.0 * np.array([[-(0.09 + 1.44 - 4) * 0.3,
                                                                          -(0.09 + 1.44 - 4) * -1.2 - 2 * (-1.2 - 1)]]))
  assert np.allclose(fp.drift(x[:, :2], "nongradient", 2.0), -2.0 * x[:, :2] + 0.5 * x[:, :2] @ np.array([[0, 1], [-1, 0]]))
  assert np.allclose(fp.drift(x, "lorenz", 1.0), [[10 * (-1.2 - 0.3), 9 * 0.3 * (28 / 9 - 2.0) + 1.2,
                                                   9 * 0.3 * -1.2 - 2.0 * 8 / 3]])
  A = fp.linear_drift_matrix("nongradient", 2.0, 2)
  assert np.allclose(fp.drift(x[:, :2], "nongradient", 2.0), x[:, :2] @ A.T)


def test_cell_rule_and_stats():
  lo, step, n = -1.0, 0.5, 5                             # points -1, -0.5, 0, 0.5, 1: cells [-1.25, -0.75), ...
  x = np.array([-1.25, -1.2500001, -0.75, -0.7500001, 0.0, 1.2499, 1.25, np.nan])
  j, ok = fp.cell_index(x, lo, step, n)
  assert ok.tolist() == [True, False, True, True, True, True, False, False]
  assert j[ok].tolist() == [0, 1, 0, 2, 4]
  pos = np.array([[[0.0, 0.1], [0.6, -0.9], [np.nan, 0.0], [9.0, 0.0], [np.inf, 1.0]]])
  grid = dict(lo=(-1.0, -1.0), step=(0.5, 0.5), n=(5, 4), axes=(0, 1))
  sums, hist = fp.stats(pos, grid)
  assert sums[0, :2].tolist() == [3, 2] and np.allclose(sums[0, 2:4], [9.6, -0.8])
  assert np.allclose(sums[0, 4:].reshape(2, 2), [[0.36 + 81, -0.54], [-0.54, 0.01 + 0.81]])
  assert hist.shape == (1, 4, 5) and hist.sum() == 2 and hist[0, 2, 2] == 1 and hist[0, 0, 3] == 1


def test_c_abi_declares_and_binds_the_entry_points():
  from cnf_ot_amd import _capi, build
  import os
  header = open(os.path.join(os.path.dirname(_capi.__file__), "..", "include", "cnf_ot_amd.h")).read()
  for name in ("cnf_fp_particles_workspace", "cnf_fp_particles", "cnf_point_stats"):
    assert name in _capi.SYMBOLS and f"int {name}(" in header
    assert hasattr(_capi.lib(), name)
  assert "cnf_fp_particles.hip" in build.SOURCES


def test_invalid_arguments_are_refused_on_the_host():
  """Every refusal happens before any device work (fake device pointers are never dereferenced)."""
  from cnf_ot_amd import _capi
  C = _capi.ctypes
  lib = _capi.lib()
  nb = C.c_int64(-1)
  assert lib.cnf_fp_particles_workspace(1000, 3, 4, C.byref(nb)) == _capi.CNF_OK
  assert nb.value == 4 * (2 + 3 + 9) * 4 * 8                      # S x terms x chunks of 256 x double
  for bad in ((0, 3, 4), (-1, 3, 4), (1000, 0, 4), (1000, 15, 4), (1000, 3, 0), (1000, 3, 65), ((1 << 31) + 1, 3, 4)):
    assert lib.cnf_fp_particles_workspace(*bad, C.byref(nb)) == _capi.CNF_ERR_INVALID, bad
  assert lib.cnf_fp_particles_workspace(1000, 3, 4, None) == _capi.CNF_ERR_INVALID

  fake = 0x1000
  lib.cnf_fp_particles_workspace(1000, 2, 3, C.byref(nb))
  grid = dict(lo_x=-1.0, lo_y=-1.0, step_x=0.5, step_y=0.5, nx=5, ny=4, axis_x=0, axis_y=1)
  good = dict(drift=0, D=2, a=1.0, sigma=0.5, h=0.01, n_steps=10, var0=1.0, seed=1, first=0, N=1000, x0=None,
              snaps=(0, 5, 10), S=3, grid=grid, pos=fake, sums=fake, hist=fake, ws=fake, wsb=nb.value)

  def c_grid(g):
    return None if g is None else C.byref(_capi.CnfFieldGrid(g["lo_x"], g["lo_y"], g["step_x"], g["step_y"], g["nx"],
                                                              g["ny"], g["axis_x"], g["axis_y"], -1, 1, None, None))

  def call(**kw):
    a = dict(good, **kw)
    snaps = None if a["snaps"] is None else (C.c_int64 * len(a["snaps"]))(*a["snaps"])
    return lib.cnf_fp_particles(a["drift"], a["D"], a["a"], a["sigma"], a["h"], a["n_steps"], a["var0"], a["seed"],
                                a["first"], a["N"], a["x0"], snaps, a["S"], c_grid(a["grid"]), a["pos"], a["sums"],
                                a["hist"], a["ws"], a["wsb"], None)

  lorenz3 = dict(drift=3, D=3)
  lib.cnf_fp_particles_workspace(1000, 3, 3, C.byref(nb))
  wsb3 = nb.value
  for bad in ({"drift": 4}, {"drift": -1},                                                  # an unknown drift
              {"drift": 1, "D": 3, "wsb": wsb3}, {"drift": 2, "D": 3, "wsb": wsb3}, {"drift": 2, "D": 1},
              {"drift": 3, "D": 2}, dict(lorenz3, D=4, wsb=1 << 30),                         # one for another dimension
              {"D": 0}, {"D": 15, "wsb": 1 << 30},
              {"h": 0.0}, {"h": -0.01}, {"h": math.nan}, {"h": math.inf},
              {"var0": 0.0}, {"var0": -1.0}, {"var0": math.nan}, {"var0": math.inf},
              {"N": 0}, {"N": -5}, {"sigma": -0.1}, {"sigma": math.nan}, {"n_steps": -1}, {"first": -1},
              {"S": 0, "snaps": ()}, {"S": 65, "snaps": tuple(range(65)), "n_steps": 100, "wsb": 1 << 30},
              {"snaps": (0, 5, 5)}, {"snaps": (5, 0, 10)}, {"snaps": (0, 5, 11)}, {"snaps": (-1, 5, 10)}, {"snaps": None},
              {"pos": None, "sums": None, "hist": None},                                    # no output
              {"grid": None},                                                               # a histogram without a grid
              {"grid": dict(grid, axis_y=0)}, {"grid": dict(grid, axis_x=2)}, {"grid": dict(grid, axis_y=-1)},
              {"grid": dict(grid, nx=0)}, {"grid": dict(grid, step_y=0.0)}, {"grid": dict(grid, lo_x=math.nan)},
              {"wsb": good["wsb"] - 8}, {"ws": None}):                                      # a workspace too small
    assert call(**bad) == _capi.CNF_ERR_INVALID, bad

  def stats(**kw):
    a = dict(good, **kw)
    return lib.cnf_point_stats(a["pos"], a["N"], a["D"], a["S"], c_grid(a["grid"]), a["sums"], a["hist"], a["ws"],
                               a["wsb"], None)

  for bad in ({"pos": None}, {"sums": None, "hist": None}, {"N": 0}, {"D": 0}, {"D": 15, "wsb": 1 << 30}, {"S": 0},
              {"S": 65, "wsb": 1 << 30}, {"grid": None}, {"grid": dict(grid, axis_y=0)}, {"grid": dict(grid, axis_x=2)},
              {"wsb": good["wsb"] - 8}, {"ws": None}):
    assert stats(**bad) == _capi.CNF_ERR_INVALID, bad


def test_python_entry_points_refuse_before_the_device():
  from cnf_ot_amd import applications as app, solvers, utils
  ok = dict(dim=2, T=1.0, a=1.0, sigma=0.5, subtype="ou", times=[0.0, 0.5], n_particles=64, h=0.01)
  for bad in ({"subtype": "rossler"}, {"subtype": "lorenz"}, {"subtype": "gradient", "dim": 3}, {"dim": 15},
              {"subtype": "nongradient", "dim": 1}, {"times": [0.0, 0.505]}, {"times": [0.5, 0.0]}, {"times": [-0.01]},
              {"times": []}, {"times": [i * 0.01 for i in range(65)]}, {"h": 0.0}, {"n_particles": 0}, {"var0": 0.0},
              {"sigma": -1.0}, {"grid": ([-1.0, 1.0, -1.0, 1.0], 10), "axes": (0, 0)},
              {"grid": ([-1.0, 1.0, -1.0, 1.0], 10), "axes": (0, 2)}, {"grid": ([-1.0, 1.0, -1.0, 1.0], 1)}):
    with pytest.raises(ValueError):
      app.fp_reference_particles(**dict(ok, **bad))
  assert app.fp_step_indices([0.0, 0.3, 1.0], 0.01, 1.0)[1].tolist() == [0, 30, 100]
  assert app.fp_initial_variance(1.0) == 1.0
  with pytest.raises(ValueError):
    utils.point_stats(np.zeros((4, 15), dtype=np.float32))
  with pytest.raises(ValueError):
    utils.point_stats(np.zeros((2, 4, 3), dtype=np.float32), grid=([-1.0, 1.0, -1.0, 1.0], 10), axes=(1, 1))
  for over in ({"general": {"type": "rwpo"}}, {"general": {"type": "ot"}}, {"general": {"type": "fp", "dim": 5}}):
    with pytest.raises(ValueError):
      solvers.evaluate_fp_path(solvers.load_config(overrides=over), None, None)
  fpc = solvers.load_config(overrides={"general": {"type": "fp"}})
  with pytest.raises(ValueError):
    solvers.evaluate_fp_path(fpc, None, None, times=[0.0, 0.0005])
  with pytest.raises(ValueError):
    solvers.evaluate_fp_path(fpc, None, None, start="data")
