"""GPU tests of cnf_hopf_cole_2d, the exact 2-D rwpo solution (cnf_ot/mfc/2d_WPO_ref_solution.py:60-187): the kernel
against the float64 restatement (tests/hopf_cole_f64.py) and the quadratic closed forms, the full-resolution true
value, evaluate()'s new keys, determinism, the argument checks, and a trained pin of the default problem.

The float64 bound: arguments <= 1e4 in magnitude and <= 2e3 terms per pass at eps = 1.1e-16 give well under 1e-11;
1e-9 leaves room for library-ulp differences in exp / log.
  log rho_T: |d| <= 1e-9 max(1, |log rho_T|);  fields: |d| <= 1e-9 max(1, max |field|);  true value, ic_mass: 1e-9
relative.
"""
import math

import numpy as np
import pytest
import torch

import hopf_cole_f64 as hc

pytestmark = pytest.mark.gpu
TOL = 1e-9
FIELDS = ("score_T", "w0", "wT")
CONFIGS = [(2.0, 10.0, 1.0), (1.0, 1.0, 0.5)]     # (T, beta, a): the default config's, and another
# The default problem (config/mfc.yaml: rwpo, double well, dim 2, T = 2, beta = 10, a = 1) at the generator's
# resolution (dz 0.01, window 6, y_range 4) and the training IC N(0, 0.6 I): hopf_cole_f64.solve, 77 s in numpy.
DEFAULT_TRUE_VAL_QUADRATURE = 0.686356378783


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def _check(got, want, what, tol=TOL, fields=FIELDS):
  lr, lw = got["log_rho_T"].cpu().numpy(), want["log_rho_T"]
  d = float((np.abs(lr - lw) / np.maximum(1.0, np.abs(lw))).max())
  msg = f"[{what}] log_rho {d:.2e}"
  assert d <= tol, (what, "log_rho_T", d)
  for k in ("true_val", "ic_mass"):
    if k in want:
      r = abs(float(got[k]) / want[k] - 1)
      msg += f" {k} {r:.2e}"
      assert r <= tol, (what, k, float(got[k]), want[k], r)
  for f in fields:
    e = float(np.abs(got[f].cpu().numpy() - want[f]).max())
    sc = max(1.0, float(np.abs(want[f]).max()))
    msg += f" {f} {e:.2e}/{sc:.3g}"
    assert e <= tol * sc, (what, f, e, sc)
  print(msg)


@pytest.mark.parametrize("dz", [0.05, 0.02])
@pytest.mark.parametrize("T,beta,a", CONFIGS)
@pytest.mark.parametrize("subtype", hc.POTENTIALS)
def test_kernel_equals_the_restatement(dev, subtype, T, beta, a, dz):
  """The generator's ranges (window 6, y_range 4); outputs on the y grid (every y in [-2, 2]) and off it (the
  reference's 100-point linspace of [-2, 2])."""
  from cnf_ot_amd import applications as app
  n = round(2.0 / dz)
  grids = {"on": np.arange(-n, n + 1) * dz, "off": np.linspace(-2.0, 2.0, 100)}
  for name, xs in grids.items():
    got = app.rwpo_reference_solution(T, beta, a, subtype, torch.tensor(xs), dz=dz)
    want = hc.solve(T, beta, a, subtype, xs, dz=dz)
    _check(got, want, f"{subtype} T={T} beta={beta} a={a} dz={dz} {name}")
    # a non-square grid: x2 a strict subset of the rows
    got = app.rwpo_reference_solution(T, beta, a, subtype, torch.tensor(xs), torch.tensor(xs[::3]), dz=dz,
                                      fields=("w0",))
    assert set(got) == {"log_rho_T", "w0", "true_val", "ic_mass"}
    want = hc.solve(T, beta, a, subtype, xs, xs[::3], dz=dz)
    _check(got, want, f"{subtype} {name} x2=x1[::3]", fields=("w0",))


@pytest.mark.parametrize("T,beta,s0,dz,window,y_range", [(1.0, 1.0, 1.0, 0.05, 12.0, 12.0),
                                                          (1.0, 4.0, 1.0, 0.05, 6.0, 10.0)])
def test_kernel_meets_the_quadratic_closed_forms(dev, T, beta, s0, dz, window, y_range):
  """rho_T = N(0, v_T I), score_T = -x / v_T, w0 = -x/(T+1) + eps x, wT = -x + eps x / v_T, true value
  2 (eps log(T+1) + s0 / (2 (T+1))) (hopf_cole_f64.closed_form), in 2-D, at wide ranges: 1e-9, relative for rho_T
  (|expm1(d log rho_T)|) and the true value, absolute for the fields."""
  from cnf_ot_amd import applications as app
  xs = np.linspace(-3.0, 3.0, 61) + 0.013
  got = app.rwpo_reference_solution(T, beta, 0.0, "quadratic", torch.tensor(xs), var0=s0, dz=dz, window=window,
                                    y_range=y_range)
  want = hc.closed_form(T, beta, s0, xs)
  what = f"closed form T={T} beta={beta} s0={s0}"
  rho = float(np.abs(np.expm1(got["log_rho_T"].cpu().numpy() - want["log_rho_T"])).max())
  tv = abs(float(got["true_val"]) / want["true_val"] - 1)
  errs = {f: float(np.abs(got[f].cpu().numpy() - want[f]).max()) for f in FIELDS}
  print(f"[{what}] rho rel {rho:.2e} true_val rel {tv:.2e} " + " ".join(f"{f} abs {e:.2e}" for f, e in errs.items()))
  assert rho <= TOL, (what, "rho_T", rho)
  assert tv <= TOL, (what, "true_val", tv)
  for f, e in errs.items():
    assert e <= TOL, (what, f, e)


def _per_x_cost_rwpo(model, params, rng, beta, T, a):
  """The 100 per-x values of cost_rwpo on evaluate's own draws (as test_evaluate_equals_its_composition redraws them)"""
  z = model.terms_backend(params).normal(rng, 100 * 1001).cpu().double().numpy()
  x = z[:100] * np.sqrt(2 / beta * (T + 1))
  y = z[100:].reshape(100, 1000, 2) * np.sqrt(2 / beta * T) + x.reshape(-1, 1, 2)
  ry = y.reshape(-1, 2)
  V = (np.linalg.norm(ry - a, axis=1) * np.linalg.norm(ry + a, axis=1) / 2) ** 2
  return -2 / beta * np.log(np.exp(V.reshape(100, 1000) * -beta / 2).mean(axis=1))


def test_full_resolution_true_value_of_the_default_problem(dev):
  """dz 0.01, window 6, y_range 4: against the recorded numpy value (1e-9); and evaluate()'s true_val_quadrature lies
  within 4 standard errors of its own Monte-Carlo true_val."""
  from cnf_ot_amd import FlowConfig, Params, applications as app, solvers
  config = solvers.load_config()
  r = config["rwpo"]
  tv = app.rwpo_true_value_quadrature(2, r["T"], r["beta"], r["a"], r["pot_type"])
  print(f"[full resolution] true_val_quadrature {tv:.12f} recorded {DEFAULT_TRUE_VAL_QUADRATURE:.12f}")
  assert abs(tv / DEFAULT_TRUE_VAL_QUADRATURE - 1) <= TOL
  model = solvers.build_model(config)
  params = Params.random(FlowConfig(dim=2), 0.2, seed=4, device=dev)
  rng = 1234
  res = solvers.evaluate(config, model, params, rng)
  per_x = _per_x_cost_rwpo(model, params, rng, r["beta"], r["T"], r["a"])
  se = per_x.std(ddof=1) / math.sqrt(per_x.size)
  print(f"[cost_rwpo] true_val {res['true_val']:.6f} (numpy {per_x.mean():.6f}) se {se:.4f}; quadrature "
        f"{res['true_val_quadrature']:.6f}: {(res['true_val_quadrature'] - res['true_val']) / se:+.2f} se; "
        f"ic_mass {res['ic_mass']:.8f}")
  assert abs(res["true_val"] - per_x.mean()) <= 1e-10 * abs(per_x.mean())
  assert abs(res["true_val_quadrature"] - res["true_val"]) <= 4 * se


def _rel(a, b):
  return abs(a - b) / max(abs(b), 1e-300)


def test_evaluate_new_keys_equal_their_composition(dev):
  """At the default config: each new key equals its composition from the public functions (1e-12), the existing keys
  keep their values, repeated calls give the same new keys bit for bit; dim 2 for every potential, None at dim 3."""
  from cnf_ot_amd import FlowConfig, Params, applications as app, solvers, utils
  rng = 1234
  config = solvers.load_config()
  r = config["rwpo"]
  T, beta, a, sub = r["T"], r["beta"], r["a"], r["pot_type"]
  model = solvers.build_model(config)
  params = Params.random(FlowConfig(dim=2), 0.2, seed=4, device=dev)
  res = solvers.evaluate(config, model, params, rng)
  print(f"[evaluate] {res}")
  assert set(res) == {"param_count", "e_kin", "e_pot", "total", "true_val", "rel_err_pct"} | set(
    solvers.RWPO_QUADRATURE_KEYS)
  # the existing keys, composed as before
  e_kin = T * float(utils.calc_score_kinetic_energy(model.apply.sample, model.apply.log_prob, params, T, beta, 2, rng))
  e_pot = float(app.potential_loss_fn(model, 2, a, sub, params, T, rng, 65536))
  true_val = app.rwpo_true_value(2, T, beta, a, sub, rng)
  assert _rel(res["e_kin"], e_kin) <= 1e-12 and _rel(res["e_pot"], e_pot) <= 1e-12
  assert res["total"] == res["e_kin"] + res["e_pot"]
  assert res["true_val"] == true_val and res["rel_err_pct"] == (res["total"] - true_val) / true_val * 100
  # the new keys from the public functions
  tv = app.rwpo_true_value_quadrature(2, T, beta, a, sub)
  xs = torch.linspace(-2.0, 2.0, 100, dtype=torch.float64).to(torch.float32)
  sol = app.rwpo_reference_solution(T, beta, a, sub, xs.double(), fields=())
  X, Y = torch.meshgrid(xs, xs, indexing="xy")
  XY = torch.stack([X.reshape(-1), Y.reshape(-1)], 1).to(dev)
  prob1 = torch.exp(model.apply.log_prob(params, XY, cond=float(T)).double())
  prob2 = torch.exp(sol["log_rho_T"].reshape(-1))
  err = float(((prob1 - prob2) ** 2).sum())
  print(f"[composition] tv {tv:.12f} density_sq_err {err:.6e} sum rho_T^2 {float((prob2 ** 2).sum()):.2f} "
        f"max rho_T {float(prob2.max()):.8f} ic_mass {float(sol['ic_mass']):.8f}")
  assert _rel(res["true_val_quadrature"], tv) <= 1e-12
  assert _rel(res["rel_err_pct_quadrature"], (res["total"] - tv) / tv * 100) <= 1e-12
  assert _rel(res["density_sq_err"], err) <= 1e-12
  assert _rel(res["ic_mass"], float(sol["ic_mass"])) <= 1e-12
  again = solvers.evaluate(config, model, params, rng)
  for k in solvers.RWPO_QUADRATURE_KEYS:
    assert again[k] == res[k], k
  # every potential at dim 2; None at dim 3
  for pot in ("quadratic", "obstacle"):
    c = solvers.load_config(overrides={"rwpo": {"pot_type": pot}})
    rp = solvers.evaluate(c, model, params, rng)
    tvp = app.rwpo_true_value_quadrature(2, T, beta, a, pot)
    print(f"[evaluate {pot}] true_val {rp['true_val']} quadrature {rp['true_val_quadrature']:.10f}")
    assert rp["true_val_quadrature"] == tvp and all(rp[k] is not None for k in solvers.RWPO_QUADRATURE_KEYS)
  assert rp["true_val"] is None          # obstacle: the Monte-Carlo value is still absent
  c3 = solvers.load_config(overrides={"general": {"dim": 3}, "rwpo": {"pot_type": "quadratic"}})
  r3 = solvers.evaluate(c3, solvers.build_model(c3), Params.random(FlowConfig(dim=3), 0.2, seed=4, device=dev), rng)
  assert all(r3[k] is None for k in solvers.RWPO_QUADRATURE_KEYS)


def test_repeated_calls_are_bit_identical(dev):
  from cnf_ot_amd import applications as app
  xs = torch.linspace(-2.0, 2.0, 100, dtype=torch.float64)
  one = app.rwpo_reference_solution(2.0, 10.0, 1.0, "double_well", xs, dz=0.02)
  two = app.rwpo_reference_solution(2.0, 10.0, 1.0, "double_well", xs, dz=0.02)
  for k in one:
    assert torch.equal(one[k], two[k]), k
  assert all(bool(torch.isfinite(v).all()) for v in one.values())


def test_invalid_arguments_are_refused_and_nothing_is_written(dev):
  from cnf_ot_amd import _capi, applications as app
  lib = _capi.lib()
  C = _capi.ctypes
  n = 8
  xs = torch.linspace(-1.0, 1.0, n, dtype=torch.float64, device=dev)
  nb = C.c_int64(0)
  assert lib.cnf_hopf_cole_workspace(0.1, 2.0, 2.0, n, n, C.byref(nb)) == _capi.CNF_OK
  ws = torch.empty(nb.value // 8, dtype=torch.float64, device=dev)
  out = {k: torch.full(s, 7.25, dtype=torch.float64, device=dev)
         for k, s in (("lr", (n, n)), ("sc", (n, n, 2)), ("w0", (n, n, 2)), ("wT", (n, n, 2)), ("tv", (2,)))}
  good = dict(subtype=1, a=1.0, T=2.0, beta=10.0, var0=0.6, dz=0.1, window=2.0, y_range=2.0, x1=xs.data_ptr(), n1=n,
              x2=xs.data_ptr(), n2=n, lr=out["lr"].data_ptr(), sc=out["sc"].data_ptr(), w0=out["w0"].data_ptr(),
              wT=out["wT"].data_ptr(), tv=out["tv"].data_ptr(), mass=out["tv"].data_ptr() + 8, ws=ws.data_ptr(),
              wsb=nb.value)

  def call(**kw):
    p = dict(good, **kw)
    return lib.cnf_hopf_cole_2d(p["subtype"], p["a"], p["T"], p["beta"], p["var0"], p["dz"], p["window"],
                                p["y_range"], p["x1"], p["n1"], p["x2"], p["n2"], p["lr"], p["sc"], p["w0"], p["wT"],
                                p["tv"], p["mass"], p["ws"], p["wsb"], None)

  for bad in ({"T": 0.0}, {"T": -2.0}, {"beta": 0.0}, {"beta": -1.0}, {"dz": 0.0}, {"dz": -0.1}, {"window": 0.0},
              {"window": -2.0}, {"var0": 0.0}, {"subtype": 3}, {"subtype": -1}, {"dz": 1e-12}, {"n1": 1 << 40},
              {"x1": None}, {"x2": None}, {"lr": None}, {"ws": None}, {"wsb": nb.value - 8}):
    assert call(**bad) == _capi.CNF_ERR_INVALID, bad
  torch.cuda.synchronize()
  assert all(bool((v == 7.25).all()) for v in out.values())
  assert call() == _capi.CNF_OK
  torch.cuda.synchronize()
  assert all(bool(torch.isfinite(v).all()) and not bool((v == 7.25).any()) for v in out.values())
  with pytest.raises(ValueError):
    app.rwpo_reference_solution(2.0, 10.0, 1.0, "mexican_hat", xs)
  with pytest.raises(_capi.CnfError):
    app.rwpo_reference_solution(0.0, 10.0, 1.0, "double_well", xs)
  with pytest.raises(ValueError):
    app.rwpo_true_value_quadrature(3, 2.0, 10.0, 1.0, "double_well")


# Regression guards of the trained default problem (30 000 captured steps): twice the first observed values (26.41 and
# 7.565), in the style of test_gpu_evaluate's pins -- not derived bounds.
DENSITY_SQ_ERR_BOUND = 52.8
REL_ERR_PCT_QUADRATURE_BOUND = 15.1


def test_trained_default_problem_against_the_exact_solution(dev):
  """The checked-in default problem trained for the reference's 30 000 epochs: its density_sq_err beats that of the
  untrained identity flow (N(0, I): measured 320.05 in numpy, sum rho_T^2 = 365.5), and density_sq_err and
  |rel_err_pct_quadrature| stay under twice their first observed values.  First observed on the MI355X (evaluation
  rng 7, 4.9 s): density_sq_err 26.41 against the identity flow's 320.05; total 0.7383 against the quadrature value
  0.686356, rel_err_pct_quadrature 7.565 (the Monte-Carlo true_val of the same run, 0.7222, gives rel_err_pct 2.22:
  its +-3 % noise hid most of the gap)."""
  import time
  from cnf_ot_amd import solvers
  t0 = time.time()
  config = solvers.load_config()
  model, params, hist = solvers.train(config, epochs=30000, capture=True)
  res = solvers.evaluate(config, model, params, 7)
  r = config["rwpo"]
  xs, pts = solvers.density_eval_points(dev)
  sol = __import__("cnf_ot_amd").applications.rwpo_reference_solution(r["T"], r["beta"], r["a"], r["pot_type"], xs,
                                                                       fields=())
  p_id = torch.exp(-(pts.double() ** 2).sum(1) / 2) / (2 * math.pi)
  err_id = float(((p_id - torch.exp(sol["log_rho_T"].reshape(-1))) ** 2).sum())
  print(f"[pin rwpo default] density_sq_err {res['density_sq_err']:.4f} (identity flow {err_id:.4f}); "
        f"rel_err_pct_quadrature {res['rel_err_pct_quadrature']:.4f}; rel_err_pct {res['rel_err_pct']:.4f}; {res} "
        f"({time.time() - t0:.1f} s)")
  assert res["density_sq_err"] < err_id
  assert res["density_sq_err"] <= DENSITY_SQ_ERR_BOUND
  assert abs(res["rel_err_pct_quadrature"]) <= REL_ERR_PCT_QUADRATURE_BOUND
