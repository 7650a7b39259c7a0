"""CPU tests of the 2-D Hopf-Cole reference solution: the float64 restatement (tests/hopf_cole_f64.py) that the GPU
tests hold cnf_hopf_cole_2d to, pinned against the direct double sum and the quadratic potential's closed forms, and
the host-side argument checks of the C ABI and the Python entry points (no device is touched).

Bounds: the restatement and the direct sum are both float64 and differ only in summation order: 1e-12 (relative for
rho_T, the true value and the IC mass; for the fields, scaled by max(1, max |field|)).  The closed forms hold
for the discrete quadrature at the inputs below to 1e-11 (relative for rho_T and the true value, absolute for the
fields): a property of the quadrature at these wide ranges, not of any code under test."""
import math

import numpy as np
import pytest

import hopf_cole_f64 as hc

FIELDS = ("score_T", "w0", "wT")
XS = np.linspace(-3.0, 3.0, 13) + 0.037           # off the y grid
CONFIGS = [(2.0, 10.0, 1.0), (1.0, 1.0, 0.5)]     # (T, beta, a): the default config's, and another


def _compare(got, want, tol, what, scaled=True):
  """rho_T, the true value and the IC mass relative; the fields absolute, against tol * max(1, max |field|) when
  `scaled` (the direct-sum comparison) and against tol itself otherwise (the closed forms)"""
  rho = float(np.abs(np.expm1(got["log_rho_T"] - want["log_rho_T"])).max())
  print(f"[{what}] rho rel {rho:.2e}", end="")
  assert rho <= tol, (what, "rho", rho)
  for k in ("true_val", "ic_mass"):
    if k in want:
      r = abs(got[k] / want[k] - 1)
      print(f" {k} rel {r:.2e}", end="")
      assert r <= tol, (what, k, r)
  for f in FIELDS:
    e = float(np.abs(got[f] - want[f]).max())
    sc = max(1.0, float(np.abs(want[f]).max())) if scaled else 1.0
    print(f" {f} {e:.2e} (scale {sc:.3g})", end="")
    assert e <= tol * sc, (what, f, e, sc)
  print()


@pytest.mark.parametrize("subtype", hc.POTENTIALS)
@pytest.mark.parametrize("T,beta,a", CONFIGS)
def test_separable_restatement_equals_the_direct_sum(subtype, T, beta, a):
  """dz 0.2 with the generator's ranges (window 6, y_range 4): 3.7e6 terms per h sweep."""
  got = hc.solve(T, beta, a, subtype, XS, dz=0.2)
  want = hc.direct(T, beta, a, subtype, XS, dz=0.2)
  _compare(got, want, 1e-12, f"{subtype} T={T} beta={beta} a={a} dz=0.2")


def test_separable_restatement_equals_the_direct_sum_at_dz_0_1():
  """The default problem at dz 0.1: 9.6e7 terms in the direct h sums, the bound's limit of 1e8."""
  xs = np.linspace(-2.0, 2.0, 7) + 0.013
  got = hc.solve(2.0, 10.0, 1.0, "double_well", xs, dz=0.1)
  want = hc.direct(2.0, 10.0, 1.0, "double_well", xs, dz=0.1)
  _compare(got, want, 1e-12, "double_well default dz=0.1")


# (T, beta, s0, dz, window, y_range): case 1 with window = y_range = 12; case 2 at the training IC s0 = 2 (T+1) / beta
CLOSED_CASES = [(1.0, 1.0, 1.0, 0.05, 12.0, 12.0), (1.0, 4.0, 1.0, 0.05, 6.0, 10.0)]


@pytest.mark.parametrize("T,beta,s0,dz,window,y_range", CLOSED_CASES)
def test_restatement_meets_the_quadratic_closed_forms(T, beta, s0, dz, window, y_range):
  xs = np.linspace(-3.0, 3.0, 25) + 0.013
  got = hc.solve(T, beta, 0.0, "quadratic", xs, var0=s0, dz=dz, window=window, y_range=y_range)
  _compare(got, hc.closed_form(T, beta, s0, xs), 1e-11, f"closed form T={T} beta={beta} s0={s0}", scaled=False)


def test_closed_form_true_value_at_the_training_ic_is_rwpo_true_value():
  """At s0 = 2 (T+1) / beta the closed form is the one rwpo_true_value pins, dim (1 + log(T+1)) / beta."""
  from cnf_ot_amd import applications as app
  for T, beta in ((2.0, 10.0), (1.0, 1.0), (1.0, 4.0)):
    s0 = app.rwpo_initial_variance(T, beta)
    cf = hc.closed_form(T, beta, s0, [0.0])["true_val"]
    assert abs(cf - app.rwpo_true_value(2, T, beta, 0.0, "quadratic")) <= 1e-15 * cf


def test_c_abi_declares_and_binds_the_entry_points():
  from cnf_ot_amd import _capi
  import os
  header = open(os.path.join(os.path.dirname(_capi.__file__), "..", "include", "cnf_ot_amd.h")).read()
  for name in ("cnf_hopf_cole_workspace", "cnf_hopf_cole_2d"):
    assert name in _capi.SYMBOLS and f"int {name}(" in header
    assert hasattr(_capi.lib(), name)


def test_workspace_query_and_invalid_arguments_on_the_host():
  """Every refusal happens before any device work, so the checks run without a GPU (fake device pointers are never
  dereferenced)."""
  from cnf_ot_amd import _capi
  C = _capi.ctypes
  lib = _capi.lib()
  nb = C.c_int64(-1)
  assert lib.cnf_hopf_cole_workspace(0.01, 6.0, 4.0, 100, 100, C.byref(nb)) == _capi.CNF_OK
  ny, nw, n = 400, 600, 100
  Ny, Nz = 2 * ny + 1, 2 * (ny + nw) + 1
  assert nb.value == 8 * (Nz * Nz + Ny * Nz + Ny * Ny + 4 * n * Ny + 6 * n * n)
  assert lib.cnf_hopf_cole_workspace(0.01, 6.0, 4.0, 0, 0, C.byref(nb)) == _capi.CNF_OK
  assert nb.value == 8 * (Nz * Nz + Ny * Nz + Ny * Ny)
  for bad in ((0.0, 6.0, 4.0, 1, 1), (-0.01, 6.0, 4.0, 1, 1), (0.01, 0.0, 4.0, 1, 1), (0.01, -6.0, 4.0, 1, 1),
              (0.01, 6.0, 0.0, 1, 1), (1e-9, 6.0, 4.0, 1, 1), (0.01, 1e9, 4.0, 1, 1), (0.01, 6.0, 4.0, 1, 0),
              (0.01, 6.0, 4.0, -1, -1), (0.01, 6.0, 4.0, 1 << 20, 1), (math.nan, 6.0, 4.0, 1, 1),
              (0.01, math.inf, 4.0, 1, 1)):
    assert lib.cnf_hopf_cole_workspace(*bad, C.byref(nb)) == _capi.CNF_ERR_INVALID, bad
  assert lib.cnf_hopf_cole_workspace(0.01, 6.0, 4.0, 1, 1, None) == _capi.CNF_ERR_INVALID

  fake = 0x1000           # never dereferenced: every call below is refused first
  lib.cnf_hopf_cole_workspace(0.2, 6.0, 4.0, 4, 4, C.byref(nb))
  good = dict(subtype=1, a=1.0, T=2.0, beta=10.0, var0=0.6, dz=0.2, window=6.0, y_range=4.0, x1=fake, n1=4, x2=fake,
              n2=4, log_rho=fake, score=None, w0=None, wT=None, tv=None, mass=None, ws=fake, wsb=nb.value, stream=None)

  def call(**kw):
    a = dict(good, **kw)
    return lib.cnf_hopf_cole_2d(a["subtype"], a["a"], a["T"], a["beta"], a["var0"], a["dz"], a["window"],
                                a["y_range"], a["x1"], a["n1"], a["x2"], a["n2"], a["log_rho"], a["score"], a["w0"],
                                a["wT"], a["tv"], a["mass"], a["ws"], a["wsb"], a["stream"])

  for bad in ({"T": 0.0}, {"T": -1.0}, {"T": math.nan}, {"beta": 0.0}, {"beta": -10.0}, {"var0": 0.0},
              {"dz": 0.0}, {"dz": -0.2}, {"window": 0.0}, {"window": -6.0}, {"y_range": -4.0}, {"subtype": 3},
              {"subtype": -1}, {"dz": 1e-12}, {"n1": 1 << 30}, {"n2": 0}, {"x1": None}, {"x2": None},
              {"log_rho": None}, {"ws": None}, {"wsb": nb.value - 8}, {"n1": 0, "n2": 0, "x1": None, "x2": None,
                                                                        "log_rho": None, "score": fake}):
    assert call(**bad) == _capi.CNF_ERR_INVALID, bad


def test_python_entry_points_refuse_before_the_device():
  from cnf_ot_amd import applications as app
  with pytest.raises(ValueError):
    app.rwpo_true_value_quadrature(3, 2.0, 10.0, 1.0, "double_well")
  with pytest.raises(ValueError):
    app.rwpo_true_value_quadrature(1, 2.0, 10.0, 1.0, "quadratic")
  with pytest.raises(ValueError):
    app.rwpo_reference_solution(2.0, 10.0, 1.0, "double_well", [0.0], fields=("rho",))
