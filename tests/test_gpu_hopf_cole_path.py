"""GPU tests of cnf_hopf_cole_path_2d, the exact 2-D rwpo solution at every time of [0, T]: the kernel against the float64
restatement (tests/hopf_cole_path_f64.py) and the quadratic closed form, the t = T slab against cnf_hopf_cole_2d bit
for bit, a batched call against one call per time, determinism, graph replay, the argument checks and
solvers.evaluate_path against its composition.

The float64 bound is test_gpu_hopf_cole's: arguments <= 1e4 in magnitude and <= 2e3 terms per pass at eps = 1.1e-16 give
well under 1e-11; 1e-9 leaves room for library-ulp differences in exp / log.
  log rho_t: |d| <= 1e-9 max(1, |log rho_t|);  fields: |d| <= 1e-9 max(1, max |field|).
"""
import math

import numpy as np
import pytest
import torch

import hopf_cole_f64 as hc
import hopf_cole_path_f64 as hp

pytestmark = pytest.mark.gpu
TOL = 1e-9
CONFIGS = [(2.0, 10.0, 1.0), (1.0, 1.0, 0.5)]     # (T, beta, a): the default config's, and another
CHUNK = 8                                         # interior times per launch (HC_TIMES)


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def _times(T):
  return (0.0, 0.3 * T, 0.85 * T, T)


def _check(got, want, what, fields=hp.FIELDS, tol=TOL):
  lr, lw = got["log_rho"].cpu().numpy(), want["log_rho"]
  assert lr.shape == lw.shape
  d = float((np.abs(lr - lw) / np.maximum(1.0, np.abs(lw))).max())
  msg = f"[{what}] log_rho {d:.2e}"
  assert d <= tol, (what, "log_rho", d)
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
  """The generator's ranges (window 6, y_range 4), times (0, 0.3 T, 0.85 T, T); outputs on the y grid (every 0.1 in
  [-2, 2]), off it (the reference's 100-point linspace of [-2, 2]), and on a non-square grid with one field.  One numpy
  solve on the union of both coordinate sets serves all three: a separable sum's value at a point does not depend on
  the other points."""
  from cnf_ot_amd import applications as app
  on = np.arange(-20, 21) * round(0.1 / dz) * dz
  off = np.linspace(-2.0, 2.0, 100)
  want = hp.solve(T, beta, a, subtype, _times(T), np.concatenate([on, off]), dz=dz)
  cut = lambda s1, s2: {k: (v[:, s2][:, :, s1] if np.ndim(v) else v) for k, v in want.items()}
  what = f"{subtype} T={T} beta={beta} a={a} dz={dz}"
  for name, xs, sl in (("on", on, slice(0, 41)), ("off", off, slice(41, None))):
    got = app.rwpo_reference_path(T, beta, a, subtype, _times(T), torch.tensor(xs), dz=dz)
    assert set(got) == {"log_rho", "score", "drift", "vel", "true_val", "ic_mass"}
    _check(got, cut(sl, sl), f"{what} {name}")
    for k in ("true_val", "ic_mass"):
      assert abs(float(got[k]) / want[k] - 1) <= TOL, k
  got = app.rwpo_reference_path(T, beta, a, subtype, _times(T), torch.tensor(off), torch.tensor(off[::3]), dz=dz,
                                fields=("vel",))
  assert set(got) == {"log_rho", "vel", "true_val", "ic_mass"} and got["vel"].shape == (4, 34, 100, 2)
  _check(got, cut(slice(41, None), slice(41, None, 3)), f"{what} x2=x1[::3]", fields=("vel",))


@pytest.mark.parametrize("T,beta,s0,dz,window,y_range", [(1.0, 1.0, 1.0, 0.05, 12.0, 12.0),
                                                          (1.0, 4.0, 1.0, 0.05, 6.0, 10.0)])
def test_kernel_meets_the_quadratic_closed_form(dev, T, beta, s0, dz, window, y_range):
  """rho_t = N(0, v_t I), score = -x / v_t, drift = -x / u, vel = -x / u + eps x / v_t (hopf_cole_path_f64.closed_form)
  at wide ranges: 1e-9, relative for rho_t (|expm1(d log rho_t)|), absolute for the fields."""
  from cnf_ot_amd import applications as app
  xs = np.linspace(-3.0, 3.0, 61) + 0.013
  got = app.rwpo_reference_path(T, beta, 0.0, "quadratic", _times(T), torch.tensor(xs), var0=s0, dz=dz, window=window,
                                y_range=y_range)
  want = hp.closed_form(T, beta, s0, _times(T), xs)
  rho = float(np.abs(np.expm1(got["log_rho"].cpu().numpy() - want["log_rho"])).max())
  errs = {f: float(np.abs(got[f].cpu().numpy() - want[f]).max()) for f in hp.FIELDS}
  print(f"[closed form T={T} beta={beta} s0={s0}] rho rel {rho:.2e} " + " ".join(f"{f} abs {e:.2e}" for f, e in errs.items()))
  assert rho <= TOL, ("rho_t", rho)
  for f, e in errs.items():
    assert e <= TOL, (f, e)


@pytest.mark.parametrize("subtype", hc.POTENTIALS)
def test_the_slab_at_T_is_the_T_solution_bit_for_bit(dev, subtype):
  from cnf_ot_amd import applications as app
  T, beta, a = CONFIGS[0]
  xs = torch.linspace(-2.0, 2.0, 100, dtype=torch.float64)
  sol = app.rwpo_reference_solution(T, beta, a, subtype, xs, xs[::3], dz=0.05)
  path = app.rwpo_reference_path(T, beta, a, subtype, (T, 0.4 * T, 0.0, T), xs, xs[::3], dz=0.05)
  for s in (0, 3):
    assert torch.equal(path["log_rho"][s], sol["log_rho_T"])
    assert torch.equal(path["score"][s], sol["score_T"]) and torch.equal(path["vel"][s], sol["wT"])
  assert torch.equal(path["true_val"], sol["true_val"]) and torch.equal(path["ic_mass"], sol["ic_mass"])
  # t = 0 is rho0 itself; vel(0) - w0 = eps x (1 / var0 - 1)
  X1, X2 = np.meshgrid(xs.numpy(), xs[::3].numpy())
  x, var0 = np.stack([X1, X2], -1), 2 * (T + 1) / beta
  assert np.abs(path["score"][2].cpu().numpy() + x / var0).max() <= 1e-15 * 2 / var0
  d = path["vel"][2].cpu().numpy() - sol["w0"].cpu().numpy() - x / beta * (1 / var0 - 1)
  assert np.abs(d).max() <= 1e-13


@pytest.mark.parametrize("S", [5, CHUNK + 1, 2 * CHUNK + 3])
def test_a_batched_call_equals_one_call_per_time(dev, S):
  """Per-time kappa, slab offsets and chunk boundaries: S = 5 inside one chunk, one above the chunk size, and three
  chunks with the endpoints in the middle of the array."""
  from cnf_ot_amd import applications as app
  T, beta, a = CONFIGS[0]
  xs = torch.linspace(-2.0, 2.0, 150, dtype=torch.float64)      # two destination blocks
  ts = list(np.linspace(0.05 * T, 0.97 * T, S))
  if S > 2 * CHUNK:
    ts[4], ts[11], ts[12] = T, 0.0, T
  kw = dict(dz=0.05, window=3.0, y_range=3.0)
  many = app.rwpo_reference_path(T, beta, a, "double_well", ts, xs, xs[::2], **kw)
  assert all(bool(torch.isfinite(v).all()) for v in many.values())
  for s, t in enumerate(ts):
    one = app.rwpo_reference_path(T, beta, a, "double_well", [t], xs, xs[::2], **kw)
    for k in ("log_rho",) + hp.FIELDS:
      assert torch.equal(many[k][s], one[k][0]), (k, s, t)
    assert torch.equal(many["true_val"], one["true_val"])


def test_repeated_calls_are_bit_identical(dev):
  from cnf_ot_amd import applications as app
  xs = torch.linspace(-2.0, 2.0, 100, dtype=torch.float64)
  ts = np.linspace(0.0, 2.0, 9)
  one = app.rwpo_reference_path(2.0, 10.0, 1.0, "double_well", ts, xs, dz=0.02)
  two = app.rwpo_reference_path(2.0, 10.0, 1.0, "double_well", ts, xs, dz=0.02)
  for k in one:
    assert torch.equal(one[k], two[k]), k
  assert all(bool(torch.isfinite(v).all()) for v in one.values())


def _c_call(lib, C, p):
  ts = None if p["times"] is None else (C.c_double * len(p["times"]))(*p["times"])
  return lib.cnf_hopf_cole_path_2d(p["subtype"], p["a"], p["T"], p["beta"], p["var0"], p["dz"], p["window"],
                                   p["y_range"], ts, p["S"], p["x1"], p["n1"], p["x2"], p["n2"], p["lr"], p["sc"],
                                   p["dr"], p["ve"], p["tv"], p["mass"], p["ws"], p["wsb"], p["stream"])


def _c_setup(dev, S, n, dz, window, y_range):
  from cnf_ot_amd import _capi
  lib, C = _capi.lib(), _capi.ctypes
  xs = torch.linspace(-1.0, 1.0, n, dtype=torch.float64, device=dev)
  nb = C.c_int64(0)
  assert lib.cnf_hopf_cole_path_workspace(dz, window, y_range, n, n, C.byref(nb)) == _capi.CNF_OK
  ws = torch.empty(nb.value // 8, dtype=torch.float64, device=dev)

  def outputs():
    return {k: torch.full(s, 7.25, dtype=torch.float64, device=dev)
            for k, s in (("lr", (S, n, n)), ("sc", (S, n, n, 2)), ("dr", (S, n, n, 2)), ("ve", (S, n, n, 2)),
                         ("tv", (2,)))}

  def args(out, **kw):
    return dict(dict(subtype=1, a=1.0, T=2.0, beta=10.0, var0=0.6, dz=dz, window=window, y_range=y_range, S=S,
                     x1=xs.data_ptr(), n1=n, x2=xs.data_ptr(), n2=n, lr=out["lr"].data_ptr(), sc=out["sc"].data_ptr(),
                     dr=out["dr"].data_ptr(), ve=out["ve"].data_ptr(), tv=out["tv"].data_ptr(),
                     mass=out["tv"].data_ptr() + 8, ws=ws.data_ptr(), wsb=nb.value, stream=None), **kw)

  return lib, C, outputs, args, nb.value, ws


def test_a_call_replays_from_a_graph_bit_for_bit(dev):
  """Captured on a single side stream (an allocation or a synchronisation would fail the capture)"""
  from cnf_ot_amd import _capi
  ts = tuple(np.linspace(0.0, 2.0, 11))              # both endpoints and two chunks
  lib, C, outputs, args, _, _ = _c_setup(dev, len(ts), 40, 0.1, 2.0, 2.0)
  eager, replay = outputs(), outputs()
  assert _c_call(lib, C, args(eager, times=ts, stream=torch.cuda.current_stream(dev).cuda_stream)) == _capi.CNF_OK
  torch.cuda.synchronize()
  side = torch.cuda.Stream(device=dev)
  side.wait_stream(torch.cuda.current_stream(dev))
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side):
    assert _c_call(lib, C, args(replay, times=ts, stream=side.cuda_stream)) == _capi.CNF_OK
  graph.replay()
  torch.cuda.synchronize()
  for k in eager:
    assert bool(torch.isfinite(eager[k]).all()) and not bool((eager[k] == 7.25).any()), k
    assert torch.equal(eager[k], replay[k]), k


def test_invalid_arguments_are_refused_and_nothing_is_written(dev):
  from cnf_ot_amd import _capi, applications as app
  T, beta, dz = 2.0, 10.0, 0.1
  ts = (0.0, 0.7, T)
  lib, C, outputs, args, nbytes, _ = _c_setup(dev, len(ts), 8, dz, 2.0, 2.0)
  out = outputs()
  band = (1.5 * dz) ** 2 * beta / 2              # sqrt(2 eps s) < 1.5 dz  <=>  s < band
  for bad in ({"times": (0.0, -0.1, T)}, {"times": (0.0, 0.7, T + 1e-9)}, {"times": (0.0, math.nan, T)},
              {"times": (0.0, 0.9 * band, T)}, {"times": (0.0, T - 0.9 * band, T)}, {"S": 0}, {"times": None},
              {"wsb": nbytes - 8},
              {"T": 0.0}, {"T": -2.0}, {"beta": 0.0}, {"beta": -1.0}, {"dz": 0.0}, {"dz": -0.1}, {"window": 0.0},
              {"window": -2.0}, {"var0": 0.0}, {"subtype": 3}, {"subtype": -1}, {"dz": 1e-12}, {"n1": 1 << 40},
              {"x1": None}, {"x2": None}, {"lr": None}, {"ws": None}):
    assert _c_call(lib, C, args(out, **dict({"times": ts}, **bad))) == _capi.CNF_ERR_INVALID, bad
  torch.cuda.synchronize()
  assert all(bool((v == 7.25).all()) for v in out.values())
  assert _c_call(lib, C, args(out, times=(0.0, 1.1 * band, T))) == _capi.CNF_OK       # just outside the band
  torch.cuda.synchronize()
  assert all(bool(torch.isfinite(v).all()) and not bool((v == 7.25).any()) for v in out.values())
  xs = torch.linspace(-1.0, 1.0, 8, dtype=torch.float64)
  with pytest.raises(_capi.CnfError):
    app.rwpo_reference_path(T, beta, 1.0, "double_well", [T + 0.5], xs, dz=dz, window=2.0, y_range=2.0)
  with pytest.raises(_capi.CnfError):
    app.rwpo_reference_path(T, beta, 1.0, "double_well", [1e-6], xs, dz=dz, window=2.0, y_range=2.0)
  with pytest.raises(ValueError):
    app.rwpo_reference_path(T, beta, 1.0, "double_well", [], xs)


def _rel(a, b):
  return abs(a - b) / max(abs(b), 1e-300)


def test_evaluate_path_equals_its_composition(dev):
  """Every list from the public functions (1e-12), evaluate() unchanged by it, ValueError where it is not defined."""
  from cnf_ot_amd import FlowConfig, Params, applications as app, solvers, utils
  config = solvers.load_config()
  r = config["rwpo"]
  T, beta, a, sub = r["T"], r["beta"], r["a"], r["pot_type"]
  model = solvers.build_model(config)
  params = Params.random(FlowConfig(dim=2), 0.2, seed=4, device=dev)
  before = solvers.evaluate(config, model, params, 1234)
  res = solvers.evaluate_path(config, model, params)
  after = solvers.evaluate(config, model, params, 1234)
  assert before == after and set(after) == {"param_count", "e_kin", "e_pot", "total", "true_val", "rel_err_pct"} | set(
    solvers.RWPO_QUADRATURE_KEYS)
  assert set(res) == {"times", "density_sq_err", "velocity_rel_err", "action_exact", "mass"}
  ts = np.linspace(0.0, T, 9)
  assert res["times"] == [float(t) for t in ts] and all(len(v) == 9 for v in res.values())
  xs, pts = solvers.density_eval_points(dev)
  dA = float(xs[1] - xs[0]) ** 2
  ref = app.rwpo_reference_path(T, beta, a, sub, ts, xs)
  flow = utils.eulerian_fields(model, params, pts, ts, rho=True, vel=True, dt=config["general"]["dt"])
  for s in range(9):
    rho = torch.exp(ref["log_rho"][s].reshape(-1))
    vel, drift = ref["vel"][s].reshape(-1, 2), ref["drift"][s].reshape(-1, 2)
    want = {"density_sq_err": float(((flow["rho"][s].double() - rho) ** 2).sum()),
            "velocity_rel_err": float((rho * ((flow["vel"][s].double() - vel) ** 2).sum(1)).sum()
                                      / (rho * (vel ** 2).sum(1)).sum()),
            "action_exact": float(0.5 * (rho * (drift ** 2).sum(1)).sum() * dA), "mass": float(rho.sum() * dA)}
    print(f"[evaluate_path t={ts[s]:.2f}] " + " ".join(f"{k} {res[k][s]:.6e}" for k in want))
    for k, v in want.items():
      assert _rel(res[k][s], v) <= 1e-12, (k, s, res[k][s], v)
  half = solvers.evaluate_path(config, model, params, times=[0.5, 1.5])
  assert half["times"] == [0.5, 1.5] and _rel(half["mass"][1], res["mass"][6]) <= 1e-12
  c3 = solvers.load_config(overrides={"general": {"dim": 3}, "rwpo": {"pot_type": "quadratic"}})
  with pytest.raises(ValueError):
    solvers.evaluate_path(c3, solvers.build_model(c3), Params.random(FlowConfig(dim=3), 0.2, seed=4, device=dev))
  cot = solvers.load_config(overrides={"general": {"type": "ot"}})
  with pytest.raises(ValueError):
    solvers.evaluate_path(cot, model, params)
