"""GPU tests of cnf_rwpo_particles, the particle reference of the rwpo problems: every per-particle output against the
float64 restatement (tests/rwpo_particles_f64.py) fed the device's own normals, the sums and the histogram against NumPy
on the kernel's own positions, a split ensemble, repeated calls, the call without u, the exact quadratic case, the
dim-2 quadrature, and solvers.evaluate_rwpo_particles against its composition.

Tolerances.  Kernel and restatement are both float64 and differ by operation order, FMA contraction and exp's last bits
over at most about 34 roundings per l_k and K additions: log_h within 256 2^-52 max(1, L_i), L_i the largest-magnitude
addend of any l_k of particle i in the restatement; ess within 1e-12 relative; mean_T and pos within 1e-13 max(1, |x|);
sel equal except where the restatement's nearest cumulative sum lies within 1e-12 of u times the total (at most 1
particle in 1000).  The measured errors are printed beside the bounds.
"""
import math

import numpy as np
import pytest
import torch

import fp_particles_f64 as fp
import rwpo_particles_f64 as rw

pytestmark = pytest.mark.gpu
N, K, S = 1000, 200, 4                                      # 1000: no multiple of the chunk of 256; 200: none of 64
T, BETA, A, SEED = 1.0, 4.0, 1.0, 13
TIMES = (0.0, 0.3 * T, 0.7 * T, T)
VAR0 = 2.0 * (T + 1.0) / BETA
# (potential, D, proposal: own = applications.rwpo_proposal's, plain = the Brownian kernel)
CASES = [("quadratic", 1, "own"), ("double_well", 2, "own"), ("obstacle", 3, "own"), ("double_well", 6, "own"),
         ("double_well", 2, "plain")]
GRID = dict(lo=(-1.5, -1.0), step=(0.5, 0.5), n=(7, 5), axes=(0, 1))      # leaves particles outside on every side
LOG_H_ULPS = 256.0 * 2.0 ** -52


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def _proposal(subtype, D, which, T=T, beta=BETA, a=A):
  from cnf_ot_amd import applications as app
  return app.rwpo_proposal(D, T, beta, a, subtype if which == "own" else "obstacle")


def _uniforms(n, first=0, seed=SEED):
  from cnf_ot_amd import applications as app
  return app.rwpo_selection_uniforms(first + n, seed)[first:]


def run(dev, subtype, D, prop, n=N, first=0, k=K, times=TIMES, with_u=True, grid=GRID, seed=SEED, T=T, beta=BETA, a=A,
        var0=VAR0):
  """One cnf_rwpo_particles call with every output that the arguments allow: a dict of numpy arrays"""
  from cnf_ot_amd import _capi
  lib, C = _capi.lib(), _capi.ctypes
  s = len(times)
  f64 = dict(dtype=torch.float64, device=dev)
  out = {"log_h": torch.full((n,), 7.25, **f64), "ess": torch.full((n,), 7.25, **f64),
         "mean_T": torch.full((n, D), 7.25, **f64)}
  g, ws, nb = None, None, C.c_int64(0)
  if with_u:
    out.update(sel=torch.full((n,), 77, dtype=torch.int32, device=dev), pos=torch.full((s, n, D), 7.25, **f64),
               sums=torch.full((s, 2 + D + D * D), 7.25, **f64))
    if grid is not None and D >= 2:
      g = _capi.CnfFieldGrid(grid["lo"][0], grid["lo"][1], grid["step"][0], grid["step"][1], grid["n"][0], grid["n"][1],
                             grid["axes"][0], grid["axes"][1], -1, 1, None, None)
      out["hist"] = torch.full((s, grid["n"][1], grid["n"][0]), 77, dtype=torch.int32, device=dev)
    _capi.check(lib.cnf_rwpo_particles_workspace(n, D, s, C.byref(nb)), "workspace")
    ws = torch.empty(nb.value // 8, **f64)
  u = torch.as_tensor(_uniforms(n, first, seed), device=dev) if with_u else None
  ts = np.asarray(times, dtype=np.float64)
  dptr = C.POINTER(C.c_double)
  centre = prop["centre"]
  centre = None if centre is None else np.ascontiguousarray(centre, dtype=np.float64)
  ptr = lambda name: out[name].data_ptr() if name in out else None
  rc = lib.cnf_rwpo_particles(rw.POTENTIALS[subtype], D, a, T, beta, var0, prop["shrink"], prop["prop_var"],
                              None if centre is None else centre.ctypes.data_as(dptr), k, seed, first, n,
                              None if u is None else u.data_ptr(), ts.ctypes.data_as(dptr), s,
                              None if g is None else C.byref(g), ptr("log_h"), ptr("ess"), ptr("mean_T"), ptr("sel"),
                              ptr("pos"), ptr("sums"), ptr("hist"), None if ws is None else ws.data_ptr(), nb.value, None)
  assert rc == _capi.CNF_OK, rc
  torch.cuda.synchronize()
  res = {name: v.cpu().numpy() for name, v in out.items()}
  if "hist" in res:
    res["hist"] = res["hist"].astype(np.int64)
  return res


def device_normals(dev, D, n=N, first=0, k=K, s=S, seed=SEED):
  """The particles' own normals from cnf_fill_normal, widened, flat from element first R on"""
  from cnf_ot_amd import _capi
  R = rw.stream_stride(D, k, s)
  out = torch.empty(n * R, dtype=torch.float32, device=dev)
  _capi.check(_capi.lib().cnf_fill_normal(seed, first * R, n * R, out.data_ptr(), None), "cnf_fill_normal")
  torch.cuda.synchronize()
  return out.cpu().numpy().astype(np.float64)


@pytest.fixture(scope="module")
def runs(dev):
  """Per case, computed once and left unchanged: the kernel's outputs and the restatement's"""
  out = {}
  for subtype, D, which in CASES:
    prop = _proposal(subtype, D, which)
    want = rw.reference(device_normals(dev, D), _uniforms(N), N, D, K, TIMES, subtype, A, T, BETA, VAR0, **prop)
    out[(subtype, D, which)] = dict(got=run(dev, subtype, D, prop), want=want, prop=prop)
  return out


@pytest.mark.parametrize("subtype,D,which", CASES)
def test_outputs_equal_the_restatement(runs, subtype, D, which):
  r = runs[(subtype, D, which)]
  got, want = r["got"], r["want"]
  tag = f"[{subtype} D={D} {which}]"
  assert all(np.isfinite(got[k]).all() for k in ("log_h", "ess", "mean_T", "pos"))
  # log_h
  bound = LOG_H_ULPS * np.maximum(1.0, want["L"])
  err = np.abs(got["log_h"] - want["log_h"])
  print(f"{tag} log_h: error {err.max():.3e}, worst error / bound {(err / bound).max():.3f} (L up to {want['L'].max():.3g}, "
        f"bound up to {bound.max():.3e})")
  assert (err <= bound).all()
  # ess
  rel = np.abs(got["ess"] - want["ess"]) / want["ess"]
  print(f"{tag} ess: median {np.median(want['ess']):.1f} min {want['ess'].min():.2f} of {K}; relative error {rel.max():.3e} "
        f"(bound 1e-12)")
  assert (rel <= 1e-12).all()
  # mean_T
  err = np.abs(got["mean_T"] - want["mean_T"]) / np.maximum(1.0, np.abs(want["mean_T"]))
  print(f"{tag} mean_T: error / max(1, |x|) {err.max():.3e} (bound 1e-13)")
  assert (err <= 1e-13).all()
  # sel
  differ = got["sel"] != want["sel"]
  close = want["gap"] <= 1e-12
  print(f"{tag} sel: {int(differ.sum())} differ, {int(close.sum())} within 1e-12 of a boundary; smallest gap {want['gap'].min():.3e}")
  assert not (differ & ~close).any()
  assert int(close.sum()) <= 1
  assert (got["sel"] >= 0).all() and (got["sel"] < K).all()
  # pos, on the particles whose selection is the restatement's
  same = ~differ
  tol = 1e-13 * np.maximum(1.0, np.abs(want["pos"]))
  err = np.abs(got["pos"] - want["pos"])[:, same]
  print(f"{tag} pos: error {err.max():.3e} (bound from {tol.min():.1e}), max |x| {np.abs(want['pos']).max():.3g}")
  assert (err <= tol[:, same]).all()
  assert (np.abs(got["pos"][0] - want["y"]) <= 1e-13 * np.maximum(1.0, np.abs(want["y"]))).all()
  assert (np.abs(got["pos"][3] - want["z_sel"])[same] <= (1e-13 * np.maximum(1.0, np.abs(want["z_sel"])))[same]).all()
  assert np.array_equal(got["pos"][0], want["y"])                         # the start is one exact product


@pytest.mark.parametrize("subtype,D,which", CASES)
def test_sums_and_histogram_of_the_kernels_own_positions(runs, subtype, D, which):
  got = runs[(subtype, D, which)]["got"]
  grid = GRID if D >= 2 else None
  want_sums, want_hist = fp.stats(got["pos"], grid)
  assert np.array_equal(got["sums"][:, :2], want_sums[:, :2]) and (got["sums"][:, 0] == N).all()
  rel = float((np.abs(got["sums"] - want_sums) / np.maximum(fp.abs_sums(got["pos"]), 1e-300)).max())
  print(f"[{subtype} D={D} {which}] sums: {rel:.2e} of sum |term| (bound 1e-12)")
  assert rel <= 1e-12
  if grid is not None:
    assert np.array_equal(got["hist"], want_hist)
    inside = want_hist.sum((1, 2))
    assert (inside > 0).all() and (inside < N).all()                      # some particles lie outside the grid


@pytest.mark.parametrize("subtype,D,which", [("double_well", 6, "own"), ("obstacle", 3, "own")])
def test_split_ensemble(dev, runs, subtype, D, which):
  r = runs[(subtype, D, which)]
  whole = r["got"]
  a = run(dev, subtype, D, r["prop"], n=437, first=0)
  b = run(dev, subtype, D, r["prop"], n=563, first=437)
  for name in ("log_h", "ess", "mean_T", "sel"):
    assert np.array_equal(np.concatenate([a[name], b[name]], 0), whole[name]), name
  assert np.array_equal(np.concatenate([a["pos"], b["pos"]], 1), whole["pos"])
  assert np.array_equal(a["hist"] + b["hist"], whole["hist"])
  assert np.array_equal((a["sums"] + b["sums"])[:, :2], whole["sums"][:, :2])
  rel = float((np.abs(a["sums"] + b["sums"] - whole["sums"]) / np.maximum(fp.abs_sums(whole["pos"]), 1e-300)).max())
  assert rel <= 1e-12, rel


@pytest.mark.parametrize("subtype,D,which", [("double_well", 6, "own"), ("double_well", 2, "plain")])
def test_two_calls_are_bit_identical(dev, runs, subtype, D, which):
  r = runs[(subtype, D, which)]
  again = run(dev, subtype, D, r["prop"])
  assert set(again) == set(r["got"])
  for name, v in again.items():
    assert np.array_equal(v, r["got"][name]), name


@pytest.mark.parametrize("subtype,D,which", [("double_well", 6, "own"), ("quadratic", 1, "own")])
def test_without_u(dev, runs, subtype, D, which):
  r = runs[(subtype, D, which)]
  bare = run(dev, subtype, D, r["prop"], with_u=False)
  assert set(bare) == {"log_h", "ess", "mean_T"}
  for name, v in bare.items():
    assert np.array_equal(v, r["got"][name]), name


def test_exact_quadratic_case(dev):
  """Quadratic with the matched proposal: every weight is equal, log h is its closed form, and the optimal path's
  variance and value are known"""
  from cnf_ot_amd import applications as app
  D, n, k, T_, beta = 5, 65536, 64, 1.0, 2.0
  var0 = 2.0 * (T_ + 1.0) / beta
  times = (0.0, 0.3 * T_, 0.7 * T_, T_)
  res = app.rwpo_reference_particles(D, T_, beta, 0.0, "quadratic", times, n_particles=n, n_inner=k, seed=SEED)
  prop = app.rwpo_proposal(D, T_, beta, 0.0, "quadratic")
  log_h, y = res["log_h"].cpu().numpy(), res["y"].cpu().numpy()
  worst, block = 0.0, 8192
  for i0 in range(0, n, block):                             # (the restatement's L_i, a block of particles at a time)
    want = rw.reference(device_normals(dev, D, block, i0, k, len(times)), None, block, D, k, times, "quadratic", 0.0, T_,
                        beta, var0, **prop)
    assert np.array_equal(y[i0:i0 + block], want["y"])
    bound = LOG_H_ULPS * np.maximum(1.0, want["L"])
    err = np.abs(log_h[i0:i0 + block] - rw.quadratic_log_h(want["y"], T_, beta))
    worst = max(worst, float((err / bound).max()))
    assert (err <= bound).all()
  ess = res["ess"].cpu().numpy()
  print(f"[exact quadratic] log_h against the closed form: worst error / bound {worst:.3f}; ess - K up to {np.abs(ess - k).max():.2e}")
  assert (np.abs(ess - k) <= 1e-12 * k).all()
  assert (res["count"].cpu().numpy() == n).all() and (res["bad"].cpu().numpy() == 0).all()
  cov = res["cov"].cpu().numpy()
  for s, t in enumerate(times):
    var = 2.0 * (T_ + 1.0 - t) / beta
    units = np.abs(np.diag(cov[s]) - var).max() / (var * math.sqrt(2.0 / n))
    print(f"[exact quadratic t={t:.1f}] variance {np.diag(cov[s])} against {var:.4f}: {units:.2f} standard errors")
    assert units <= 5.0
  want_val = D * (1.0 + math.log(T_ + 1.0)) / beta
  val, se = float(res["true_val"]), float(res["true_val_se"])
  print(f"[exact quadratic] true_val {val:.6f} against {want_val:.6f}: {(val - want_val) / se:+.2f} standard errors; "
        f"bias_est {float(res['bias_est']):.2e}")
  assert abs(val - want_val) <= 5.0 * se
  # the control at time 0, (mean_T - y) / T, is -y / (1 + T) up to the inner ensemble's noise: K equal weights of
  # variance prop_var per coordinate
  drift0, mean_T = res["drift0"].cpu().numpy(), res["mean_T"].cpu().numpy()
  assert np.array_equal(drift0, (mean_T - y) / T_)
  units = (drift0 + y / (1.0 + T_)).std() / (math.sqrt(prop["prop_var"] / k) / T_)
  print(f"[exact quadratic] drift0 + y / (1 + T): {units:.4f} of its standard deviation sqrt(prop_var / K) / T")
  assert abs(units - 1.0) <= 5.0 * math.sqrt(0.5 / (n * D))


@pytest.mark.parametrize("T_,beta", [(1.0, 4.0), (2.0, 10.0)])
def test_value_against_the_quadrature(dev, T_, beta):
  from cnf_ot_amd import applications as app
  plain = app.rwpo_proposal(2, T_, beta, 1.0, "obstacle")
  res = app.rwpo_reference_particles(2, T_, beta, 1.0, "double_well", (T_,), n_particles=4096, n_inner=1024, seed=SEED,
                                     proposal=plain)
  want = app.rwpo_true_value_quadrature(2, T_, beta, 1.0, "double_well")
  val, se = float(res["true_val_corrected"]), float(res["true_val_se"])
  print(f"[quadrature T={T_} beta={beta}] corrected {val:.6f} (bias {float(res['bias_est']):.2e}) against {want:.6f}: "
        f"{(val - want) / se:+.2f} standard errors (se {se:.2e}); ess median {float(res['ess'].median()):.1f}")
  assert abs(val - want) <= 5.0 * se


def test_endpoint_histogram_against_the_quadrature(dev):
  """The selected endpoints are draws of rho_T: their histogram against the cell masses of the exact dim-2 solution.  A
  half-against-half distance is twice the expected whole-against-exact one, so the margin is 2."""
  from cnf_ot_amd import applications as app
  T_, beta, n, cells = 1.0, 4.0, 65536, 40
  plain = app.rwpo_proposal(2, T_, beta, 1.0, "obstacle")
  grid = ([-3.0, 3.0, -3.0, 3.0], cells)
  halves = [app.rwpo_reference_particles(2, T_, beta, 1.0, "double_well", (T_,), n_particles=n // 2, n_inner=1024, seed=SEED,
                                         proposal=plain, grid=grid, first=h * (n // 2)) for h in (0, 1)]
  xs = np.linspace(-3.0, 3.0, cells)
  sol = app.rwpo_reference_solution(T_, beta, 1.0, "double_well", xs, fields=())
  mass = torch.exp(sol["log_rho_T"]) * (xs[1] - xs[0]) ** 2              # [ny, nx]: the midpoint rule at the cell centres
  ha, hb = halves[0]["hist"][0].double(), halves[1]["hist"][0].double()
  tv = float(0.5 * ((ha + hb) / n - mass).abs().sum())
  floor = float(0.5 * (ha / (n // 2) - hb / (n // 2)).abs().sum())
  print(f"[endpoint histogram] tv against the exact cell masses {tv:.5f}, floor of the two halves {floor:.5f}; "
        f"mass on the grid {float(mass.sum()):.6f}, counted {float((ha + hb).sum()) / n:.6f}")
  assert tv <= floor


@pytest.mark.parametrize("dim", [2, 6])
def test_evaluate_rwpo_particles_equals_its_composition(dev, dim):
  from cnf_ot_amd import FlowConfig, Params, applications as app, solvers, utils
  config = solvers.load_config(overrides={"general": {"type": "rwpo", "dim": dim}})
  r = config["rwpo"]
  model = solvers.build_model(config)
  params = Params.random(FlowConfig(dim=dim), 0.2, seed=4, device=dev)
  n, k, seed = 2048, 256, 5
  res = solvers.evaluate_rwpo_particles(config, model, params, n_particles=n, n_inner=k, seed=seed)
  per_time = {"times", "mean_err", "cov_rel_err", "tv", "tv_floor", "bad"}
  scalars = {"true_val", "true_val_se", "bias_est", "true_val_corrected", "ess_median", "ess_min"}
  assert set(res) == per_time | scalars
  ts = np.linspace(0.0, float(r["T"]), 5)
  assert res["times"] == [float(t) for t in ts] and all(len(res[name]) == 5 for name in per_time)
  grid = utils.field_grid(solvers.rwpo_particles_domain(config), 100)
  flow = utils.point_stats(torch.stack([model.apply.sample(params, cond=float(t), seed=seed, sample_shape=(n,))
                                        for t in ts]), grid)
  args = (dim, r["T"], r["beta"], r["a"], r["pot_type"], ts)
  whole = app.rwpo_reference_particles(*args, n_particles=n, n_inner=k, seed=seed, grid=grid)
  halves = [app.rwpo_reference_particles(*args, n_particles=n // 2, n_inner=k, seed=seed, grid=grid, first=h * (n // 2))
            for h in (0, 1)]
  assert (halves[0]["hist"] + halves[1]["hist"]).equal(whole["hist"])
  assert torch.cat([halves[0]["log_h"], halves[1]["log_h"]]).equal(whole["log_h"])
  for s in range(5):
    want = {"mean_err": float(torch.linalg.norm(flow["mean"][s] - whole["mean"][s])),
            "cov_rel_err": float(torch.linalg.norm(flow["cov"][s] - whole["cov"][s]) / torch.linalg.norm(whole["cov"][s])),
            "tv": float(0.5 * (flow["hist"][s] - whole["hist"][s]).abs().sum()) / n,
            "tv_floor": float(0.5 * (halves[0]["hist"][s] - halves[1]["hist"][s]).abs().sum()) / (n // 2),
            "bad": float(whole["bad"][s])}
    print(f"[evaluate_rwpo_particles dim {dim} t={ts[s]:.2f}] " + " ".join(f"{name} {res[name][s]:.4e}" for name in want))
    for name, v in want.items():
      # the moments of the whole ensemble and of its two halves differ in the last additions of their sums
      assert abs(res[name][s] - v) <= 1e-9 * max(abs(v), 1.0 if name in ("mean_err", "cov_rel_err") else 0.0), (name, s)
    assert res["tv_floor"][s] > 0.0 and res["bad"][s] == 0.0
  for name in ("true_val", "true_val_se", "bias_est", "true_val_corrected"):
    assert res[name] == float(whole[name]), name
  assert res["ess_median"] == float(whole["ess"].median()) and res["ess_min"] == float(whole["ess"].min())
  print(f"[evaluate_rwpo_particles dim {dim}] " + " ".join(f"{name} {res[name]:.5g}" for name in sorted(scalars)))
  assert 1.0 <= res["ess_min"] <= res["ess_median"] <= k * (1.0 + 1e-12)


def test_evaluate_rwpo_particles_refuses_other_problems(dev):
  from cnf_ot_amd import solvers
  for _type in ("fp", "ot"):
    config = solvers.load_config(overrides={"general": {"type": _type, "dim": 2}})
    with pytest.raises(ValueError):
      solvers.evaluate_rwpo_particles(config, None, None)
  config = solvers.load_config(overrides={"general": {"type": "rwpo", "dim": 2}})
  with pytest.raises(ValueError):
    solvers.evaluate_rwpo_particles(config, None, None, n_particles=1001)
