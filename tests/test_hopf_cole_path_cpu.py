"""CPU tests of the 2-D Hopf-Cole solution along [0, T]: the float64 restatement (tests/hopf_cole_path_f64.py) that the
GPU tests hold cnf_hopf_cole_path_2d to, pinned against the direct double sum, hopf_cole_f64.solve at t = T and the
quadratic closed form, and the host-side argument checks of the C ABI (no device is touched).

Bounds, as tests/test_hopf_cole_cpu.py sets them for t = T: restatement and direct sum are both float64 and differ only
in summation order, 1e-12 (relative for rho_t; the fields scaled by max(1, max |field|)); the closed form holds for the
discrete quadrature at the wide ranges below to 1e-11 (relative for rho_t, absolute for the fields)."""
import math

import numpy as np
import pytest

import hopf_cole_f64 as hc
import hopf_cole_path_f64 as hp

XS = np.linspace(-3.0, 3.0, 13) + 0.037           # off the y grid
CONFIGS = [(2.0, 10.0, 1.0), (1.0, 1.0, 0.5)]     # (T, beta, a): the default config's, and another


def _times(T):
  return (0.0, 0.3 * T, 0.85 * T, T)


def _compare(got, want, tol, what, scaled=True):
  rho = float(np.abs(np.expm1(got["log_rho"] - want["log_rho"])).max())
  print(f"[{what}] rho rel {rho:.2e}", end="")
  assert rho <= tol, (what, "rho", rho)
  for f in hp.FIELDS:
    e = float(np.abs(got[f] - want[f]).max())
    sc = max(1.0, float(np.abs(want[f]).max())) if scaled else 1.0
    print(f" {f} {e:.2e} (scale {sc:.3g})", end="")
    assert e <= tol * sc, (what, f, e, sc)
  print()


@pytest.mark.parametrize("subtype", hc.POTENTIALS)
@pytest.mark.parametrize("T,beta,a", CONFIGS)
def test_path_restatement_equals_the_direct_sum(subtype, T, beta, a):
  got = hp.solve(T, beta, a, subtype, _times(T), XS, dz=0.2)
  want = hp.direct(T, beta, a, subtype, _times(T), XS, dz=0.2)
  assert got["log_rho"].shape == (4, 13, 13) and got["vel"].shape == (4, 13, 13, 2)
  _compare(got, want, 1e-12, f"{subtype} T={T} beta={beta} a={a} dz=0.2")
  for k in ("true_val", "ic_mass"):
    assert abs(got[k] / want[k] - 1) <= 1e-12, k


@pytest.mark.parametrize("subtype", hc.POTENTIALS)
def test_path_restatement_at_T_is_the_T_solution(subtype):
  T, beta, a = CONFIGS[0]
  got = hp.solve(T, beta, a, subtype, (0.5 * T, T), XS, XS[::2], dz=0.1)
  want = hc.solve(T, beta, a, subtype, XS, XS[::2], dz=0.1)
  for k, kT in (("log_rho", "log_rho_T"), ("score", "score_T"), ("vel", "wT")):
    e = float(np.abs(got[k][1] - want[kT]).max())
    assert e <= 1e-13 * max(1.0, float(np.abs(want[kT]).max())), (k, e)
  X1, X2 = np.meshgrid(XS, XS[::2])
  g = hc.potential(X1, X2, subtype, a)
  assert np.array_equal(got["drift"][1], -np.stack(g[1:], -1))


# the two wide-range settings of test_hopf_cole_cpu's closed-form test, s0 = var0: the first is not 2 eps (T + 1) = 4,
# the second is the default 2 (T + 1) / beta = 1
CLOSED_CASES = [(1.0, 1.0, 1.0, 0.05, 12.0, 12.0), (1.0, 4.0, 1.0, 0.05, 6.0, 10.0)]


@pytest.mark.parametrize("T,beta,s0,dz,window,y_range", CLOSED_CASES)
def test_path_restatement_meets_the_quadratic_closed_form(T, beta, s0, dz, window, y_range):
  xs = np.linspace(-3.0, 3.0, 25) + 0.013
  got = hp.solve(T, beta, 0.0, "quadratic", _times(T), xs, var0=s0, dz=dz, window=window, y_range=y_range)
  want = hp.closed_form(T, beta, s0, _times(T), xs)
  _compare(got, want, 1e-11, f"closed form T={T} beta={beta} s0={s0}", scaled=False)
  end = hc.closed_form(T, beta, s0, xs)
  assert np.abs(want["log_rho"][-1] - end["log_rho_T"]).max() <= 1e-14
  assert np.abs(want["vel"][-1] - end["wT"]).max() <= 1e-14


def test_default_var0_is_used_and_differs_from_case_one():
  assert 2 * (1.0 + 1) / 4.0 == CLOSED_CASES[1][2] and 2 * (1.0 + 1) / 1.0 != CLOSED_CASES[0][2]
  xs = np.linspace(-1.0, 1.0, 5)
  T, beta, s0, dz, window, y_range = CLOSED_CASES[1]
  a = hp.solve(T, beta, 0.0, "quadratic", (0.0, 0.5), xs, dz=dz, window=window, y_range=y_range)
  b = hp.solve(T, beta, 0.0, "quadratic", (0.0, 0.5), xs, var0=s0, dz=dz, window=window, y_range=y_range)
  assert all(np.array_equal(a[k], b[k]) for k in ("log_rho",) + hp.FIELDS)


@pytest.mark.parametrize("var0", [0.6, 1.0, 1.7])
def test_velocity_at_0_against_w0(var0):
  """vel(0) - w0 = eps x (1 / var0 - 1): the existing w0 is the generator's drift + eps x, right for var0 = 1 only"""
  T, beta, a = CONFIGS[0]
  got = hp.solve(T, beta, a, "double_well", (0.0,), XS, var0=var0, dz=0.1)
  w0 = hc.solve(T, beta, a, "double_well", XS, var0=var0, dz=0.1)["w0"]
  X1, X2 = np.meshgrid(XS, XS)
  want = np.stack([X1, X2], -1) / beta * (1 / var0 - 1)
  assert np.abs(got["vel"][0] - w0 - want).max() <= 1e-13
  assert np.array_equal(got["score"][0], -np.stack([X1, X2], -1) / var0)


def test_c_abi_declares_and_binds_the_path_entry_points():
  from cnf_ot_amd import _capi
  import os
  header = open(os.path.join(os.path.dirname(_capi.__file__), "..", "include", "cnf_ot_amd.h")).read()
  for name in ("cnf_hopf_cole_path_workspace", "cnf_hopf_cole_path_2d"):
    assert name in _capi.SYMBOLS and f"int {name}(" in header
    assert hasattr(_capi.lib(), name)


def test_path_workspace_query_and_invalid_arguments_on_the_host():
  """Every refusal happens before any device work (fake device pointers are never dereferenced)."""
  from cnf_ot_amd import _capi
  C = _capi.ctypes
  lib = _capi.lib()
  nb, nb0 = C.c_int64(-1), C.c_int64(-1)
  assert lib.cnf_hopf_cole_path_workspace(0.01, 6.0, 4.0, 100, 100, C.byref(nb)) == _capi.CNF_OK
  assert lib.cnf_hopf_cole_workspace(0.01, 6.0, 4.0, 100, 100, C.byref(nb0)) == _capi.CNF_OK
  n, Ny, Nz = 100, 801, 2001
  assert nb.value == nb0.value + 8 * 8 * (2 * n * Nz + 2 * n * Ny + 6 * n * n)      # 8 times per chunk
  for bad in ((0.0, 6.0, 4.0, 1, 1), (0.01, 6.0, 4.0, 0, 0), (0.01, 6.0, 4.0, 1, 0), (math.nan, 6.0, 4.0, 1, 1)):
    assert lib.cnf_hopf_cole_path_workspace(*bad, C.byref(nb)) == _capi.CNF_ERR_INVALID, bad
  assert lib.cnf_hopf_cole_path_workspace(0.01, 6.0, 4.0, 1, 1, None) == _capi.CNF_ERR_INVALID

  fake = 0x1000
  lib.cnf_hopf_cole_path_workspace(0.2, 6.0, 4.0, 4, 4, C.byref(nb))
  T, beta, dz = 2.0, 10.0, 0.2
  band = (1.5 * dz) ** 2 * beta / 2              # sqrt(2 eps s) < 1.5 dz  <=>  s < band
  good = dict(subtype=1, a=1.0, T=T, beta=beta, var0=0.6, dz=dz, window=6.0, y_range=4.0, times=(0.0, 1.0, T), S=3,
              x1=fake, n1=4, x2=fake, n2=4, log_rho=fake, ws=fake, wsb=nb.value)

  def call(**kw):
    a = dict(good, **kw)
    ts = None if a["times"] is None else (C.c_double * len(a["times"]))(*a["times"])
    return lib.cnf_hopf_cole_path_2d(a["subtype"], a["a"], a["T"], a["beta"], a["var0"], a["dz"], a["window"],
                                     a["y_range"], ts, a["S"], a["x1"], a["n1"], a["x2"], a["n2"], a["log_rho"], None,
                                     None, None, None, None, a["ws"], a["wsb"], None)

  for bad in ({"times": (0.0, -0.1, T)}, {"times": (0.0, 1.0, T + 1e-9)}, {"times": (0.0, math.nan, T)},
              {"times": (0.0, math.inf, T)}, {"times": (0.0, 0.9 * band, T)}, {"times": (0.0, T - 0.9 * band, T)},
              {"S": 0}, {"S": -1}, {"times": None}, {"wsb": nb.value - 8}, {"ws": None}, {"n1": 0, "n2": 0},
              {"T": 0.0}, {"T": math.nan}, {"beta": 0.0}, {"var0": 0.0}, {"dz": 0.0}, {"window": 0.0}, {"y_range": -4.0},
              {"subtype": 3}, {"subtype": -1}, {"n2": 0}, {"x1": None}, {"x2": None}, {"log_rho": None}):
    assert call(**bad) == _capi.CNF_ERR_INVALID, bad


def test_python_entry_points_refuse_before_the_device():
  from cnf_ot_amd import applications as app, solvers
  with pytest.raises(ValueError):
    app.rwpo_reference_path(2.0, 10.0, 1.0, "double_well", [0.0, 1.0], [0.0], fields=("w0",))
  with pytest.raises(ValueError):
    app.rwpo_reference_path(2.0, 10.0, 1.0, "mexican_hat", [0.0, 1.0], [0.0])
  for over in ({"general": {"dim": 3}}, {"general": {"type": "ot"}}):
    with pytest.raises(ValueError):
      solvers.evaluate_path(solvers.load_config(overrides=over), None, None)
