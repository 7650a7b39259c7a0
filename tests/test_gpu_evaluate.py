"""GPU tests of the post-training evaluation (cnf_ot/mfc/solvers.py:129-308): the density-error terms
CNF_TERM_DENSITY_L2 (base noise) and CNF_TERM_DENSITY_L2_DATA (data points) against a float64 restatement built from
the oracle (OracleFlow, the numpy mixture of oracle/losses.py), their spec checks, sharding, the composition of
solvers.evaluate from the public functions, and closed-form pins of trained runs.

Tolerance of the terms: |sum_gpu - sum_f64| <= TOL * sum_i (p_flow_i^2 + p_mix_i^2), the scale of the residual's two
parts (the residual itself cancels where the flow fits the mixture).  fp32 log-densities carry ~1e-6 absolute error,
so exp(lp) ~1e-6 relative; measured worst case: see the printed `rel` values (expected ~1e-5).
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-4
TS = (0.0, 0.3, 1.0)
V0, A, HORIZON = 4.0, 1.0, 1.0


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def _setup(dev, D, scale, seed=3):
  import oracle
  from oracle import losses as ol
  from cnf_ot_amd import FlowConfig, FlowModel, Params
  cfg = FlowConfig(dim=D)
  model = FlowModel(cfg)
  params = Params.random(cfg, scale, seed=seed, device=dev)
  flow = ol.OracleFlow(oracle.OracleConfig(D=D), params.flat.cpu().double().numpy())
  return model, params, flow


def _mix64(y, t, v0=V0, a=A, T=HORIZON):
  from oracle.losses import _mvn_iso_pdf
  vT = math.exp(-2.0 * a * T) * (v0 - 0.5 / a) + 0.5 / a
  return (1.0 - t) * _mvn_iso_pdf(y, v0) + t * _mvn_iso_pdf(y, vT)


def _want(pf, pm):
  """(float64 sum of the residuals, the bound's scale)"""
  return float(((pf - pm) ** 2).sum()), float((pf * pf + pm * pm).sum())


def _check(name, got, want, scale, tol=TOL):
  rel = abs(float(got) - want) / scale
  print(f"[{name}] gpu={float(got):.10g} f64={want:.10g} scale={scale:.4g} rel={rel:.2e}")
  assert rel <= tol, (name, float(got), want, rel)


def _spec(kind, v0=V0, a=A, T=HORIZON):
  from cnf_ot_amd import applications as app
  return app._spec(kind, coef=v0, a=a, T=T)


def _path(be, path):
  be.set_pwl(2 if path == "tables" else 0)


# N(0, 0.5^2) parameters at dim >= 3 give log-densities of 50 .. 270 on some samples (measured: the float64 residual
# sums reach 3e21 at dim 3 and 7e117 at dim 10): exp(lp) leaves float32's range, and the kernel's fp32 residual with
# it, so that scale is held at dims 1 and 2 only.
CASES = [(D, path, s) for s in (0.2, 0.5) for D, path in ((1, "mlp"), (2, "mlp"), (3, "mlp"), (10, "mlp"), (2, "tables"))
         if s == 0.2 or D <= 2]


@pytest.mark.parametrize("D,path,scale", CASES)
def test_density_l2_base_noise_term_vs_float64(dev, D, path, scale):
  """CNF_TERM_DENSITY_L2: one base -> data pass at t, (exp(lp) - p_mix(y; t))^2 summed per slice; explicit noise and
  the seeded launch agree on the same cnf_fill_normal draws."""
  from cnf_ot_amd import _capi
  model, params, flow = _setup(dev, D, scale)
  be = model.terms_backend(params)
  _path(be, path)
  B, seed = 4096 + 37, 11
  z = be.normal(seed, B)
  spec = _spec(_capi.TERM_DENSITY_L2)
  got = be.loss_terms(spec, z, list(TS), B, True).cpu().numpy()
  assert be.last_path() == ("loss_tables" if path == "tables" else "loss_mlp")
  seeded = be.loss_terms_seeded(spec, seed, list(TS), B, first_sample=0, slice_stride=0).cpu().numpy()
  print(f"[seeded vs explicit] max rel {np.abs(seeded - got).max() / np.abs(got).max():.2e}")
  np.testing.assert_allclose(seeded, got, rtol=1e-6, atol=0)
  z64 = z.cpu().double().numpy()
  for k, t in enumerate(TS):
    y, lp = flow.sample_and_log_prob(z64, [t])
    want, sc = _want(np.exp(lp), _mix64(y, t))
    _check(f"L2 base D={D} {path} s={scale} t={t}", got[k], want, sc)
  be.set_pwl(1)


@pytest.mark.parametrize("D,path,scale", CASES)
def test_density_l2_data_term_vs_float64(dev, D, path, scale):
  """CNF_TERM_DENSITY_L2_DATA: one data -> base pass on the points, the residual at the point itself; on the
  reference's grid (dim 2) and on scattered points."""
  from cnf_ot_amd import _capi, applications as app
  model, params, flow = _setup(dev, D, scale)
  be = model.terms_backend(params)
  _path(be, path)
  sets = {"scattered": be.normal(5, 4096 + 37) * 1.5}
  if D == 2:
    sets["grid"] = app.density_grid(72, -5.0, 5.0, range(72), be.device)
  spec = _spec(_capi.TERM_DENSITY_L2_DATA)
  for what, pts in sets.items():
    got = be.loss_terms(spec, pts, list(TS), pts.shape[0], True).cpu().numpy()
    assert be.last_path() == ("loss_tables" if path == "tables" else "loss_mlp")
    x64 = pts.cpu().double().numpy()
    for k, t in enumerate(TS):
      want, sc = _want(np.exp(flow.log_prob(x64, [t])), _mix64(x64, t))
      _check(f"L2 data D={D} {path} s={scale} {what} t={t}", got[k], want, sc)
  be.set_pwl(1)


def test_density_l2_spec_checks_leave_buffers_untouched(dev):
  """coef, a, T <= 0 -> CNF_ERR_INVALID from cnf_loss_terms; the data kind from cnf_loss_terms_seeded; both kinds
  from cnf_loss_terms_grad(_multi) -- evaluation terms have no backward.  Nothing is written."""
  from cnf_ot_amd import _capi
  C = _capi.ctypes
  model, params, _ = _setup(dev, 2, 0.2)
  be = model.terms_backend(params)
  lib, h, stream = be.lib, be._h, None
  B = 512
  pts = be.normal(1, B)
  t = torch.tensor([0.5], dtype=torch.float32, device=dev)
  sums = torch.full((1,), 7.25, dtype=torch.float64, device=dev)
  grad = torch.full((params.flat.numel(),), 3.5, dtype=torch.float32, device=dev)
  _capi.check(lib.cnf_grad_enable(h, 0), "cnf_grad_enable")

  def untouched():
    torch.cuda.synchronize()
    assert float(sums[0]) == 7.25 and bool((grad == 3.5).all())

  for kind in (_capi.TERM_DENSITY_L2, _capi.TERM_DENSITY_L2_DATA):
    for bad in ({"v0": 0.0}, {"v0": -1.0}, {"a": 0.0}, {"a": -1.0}, {"T": 0.0}, {"T": -2.0}):
      spec = _spec(kind, **bad)
      assert lib.cnf_loss_terms(h, C.byref(spec), pts.data_ptr(), 1, t.data_ptr(), 1, B, sums.data_ptr(),
                                stream) == _capi.CNF_ERR_INVALID, (kind, bad)
      untouched()
    good = _spec(kind)
    r = lib.cnf_loss_terms_seeded(h, C.byref(good), 1, 0, 0, t.data_ptr(), 1, B, sums.data_ptr(), stream)
    assert r == (_capi.CNF_ERR_INVALID if kind == _capi.TERM_DENSITY_L2_DATA else _capi.CNF_OK), (kind, r)
    if r == _capi.CNF_OK:
      sums.fill_(7.25)
    untouched()
    assert lib.cnf_loss_terms_grad(h, C.byref(good), pts.data_ptr(), 1, t.data_ptr(), 1, B, 1.0, sums.data_ptr(),
                                   grad.data_ptr(), params.flat.data_ptr(), stream) == _capi.CNF_ERR_INVALID
    untouched()
    # a valid term first: the whole multi call is refused, the valid term's sums included
    specs = (_capi.CnfLossSpec * 2)(_spec(_capi.TERM_POTENTIAL, v0=0.0), good)
    ptrs = (C.c_void_p * 2)(pts.data_ptr(), pts.data_ptr())
    ts_ = (C.c_void_p * 2)(t.data_ptr(), t.data_ptr())
    ss = (C.c_void_p * 2)(sums.data_ptr(), sums.data_ptr())
    assert lib.cnf_loss_terms_grad_multi(h, 2, specs, ptrs, (C.c_int32 * 2)(1, 1), ts_, (C.c_int64 * 2)(1, 1),
                                         (C.c_int64 * 2)(B, B), (C.c_float * 2)(1.0, 1.0), ss, grad.data_ptr(),
                                         params.flat.data_ptr(), stream) == _capi.CNF_ERR_INVALID
    untouched()
  # the residual entry has no density-error form either
  for kind in (_capi.TERM_DENSITY_L2, _capi.TERM_DENSITY_L2_DATA):
    assert lib.cnf_term_residual(kind, pts.data_ptr(), pts.data_ptr(), B, B, 2, 0, 1.0, 1.0, sums.data_ptr(), None,
                                 None, stream) == _capi.CNF_ERR_INVALID
    untouched()


@pytest.mark.parametrize("path", ["mlp", "tables"])
def test_density_l2_two_rank_split_adds_up(dev, path):
  """Both ranks of a 2-way split, in one process at the engine level: the seeded term with first_sample from
  shard_range, the grid term on each rank's rows.  The partial sums add up to the single-rank sums.  The splits lie on
  tile boundaries, so on the tables the per-wave float partials are the same and only the float64 accumulation order
  differs (1e-12).  The MLP kernel packs two samples per lane from 131 072 samples on and one below, so the halves
  form other float partials (measured 1e-9 relative; bound 1e-7)."""
  from cnf_ot_amd import _capi, applications as app
  from cnf_ot_amd.distributed import Shard, shard_range
  model, params, _ = _setup(dev, 2, 0.2)
  be = model.terms_backend(params)
  _path(be, path)
  n, G, seed = 2 * 65536, 512, 21
  spec, dspec = _spec(_capi.TERM_DENSITY_L2), _spec(_capi.TERM_DENSITY_L2_DATA)
  one = float(be.loss_terms_seeded(spec, seed, [1.0], n)[0])
  grid = app.density_grid(G, -5.0, 5.0, range(G), be.device)
  one_g = float(be.loss_terms(dspec, grid, [1.0], G * G, True)[0])
  two = two_g = 0.0
  for r in range(2):
    start, count = shard_range(n, Shard(r, 2))
    two += float(be.loss_terms_seeded(spec, seed, [1.0], count, first_sample=start)[0])
    r0, rows = shard_range(G, Shard(r, 2))
    pts = app.density_grid(G, -5.0, 5.0, range(r0, r0 + rows), be.device)
    two_g += float(be.loss_terms(dspec, pts, [1.0], pts.shape[0], True)[0])
  print(f"[split {path}] mc {one:.17g} vs {two:.17g}; grid {one_g:.17g} vs {two_g:.17g}")
  tol = 1e-12 if path == "tables" else 1e-7
  assert abs(two - one) <= tol * abs(one) and abs(two_g - one_g) <= tol * abs(one_g)
  be.set_pwl(1)


def _rel(a, b):
  return abs(a - b) / max(abs(b), 1e-300)


def test_evaluate_equals_its_composition(dev):
  """Each evaluate entry equals its composition from the public functions (the fused sums are accumulated with
  float64 atomics, whose order is not fixed: agreement to 1e-12 relative rather than bit for bit); l2_mc / l2_grid
  match the float64 restatement within the terms' bound; rwpo_true_value matches a numpy cost_rwpo."""
  from oracle import losses as ol
  from cnf_ot_amd import FlowConfig, Params, applications as app, solvers, utils
  rng = 1234
  # rwpo, double well (the checked-in default)
  config = solvers.load_config()
  model = solvers.build_model(config)
  params = Params.random(FlowConfig(dim=2), 0.2, seed=4, device=dev)
  res = solvers.evaluate(config, model, params, rng)
  r = config["rwpo"]
  e_kin = r["T"] * float(utils.calc_score_kinetic_energy(model.apply.sample, model.apply.log_prob, params, r["T"],
                                                         r["beta"], 2, rng))
  e_pot = float(app.potential_loss_fn(model, 2, r["a"], r["pot_type"], params, r["T"], rng, 65536))
  assert res["param_count"] == params.flat.numel() == 1200
  assert _rel(res["e_kin"], e_kin) <= 1e-12 and _rel(res["e_pot"], e_pot) <= 1e-12, (res, e_kin, e_pot)
  assert res["total"] == res["e_kin"] + res["e_pot"]
  # cost_rwpo in numpy float64 on the same draws: x = samples 0..99, y = the next 100 000 of the stream
  z = model.terms_backend(params).normal(rng, 100 * 1001).cpu().double().numpy()
  beta, T, a = r["beta"], r["T"], r["a"]
  x = z[:100] * np.sqrt(2 / beta * (T + 1))
  y = z[100:].reshape(100, 1000, 2) * np.sqrt(2 / beta * T) + x.reshape(-1, 1, 2)
  ry = y.reshape(-1, 2)
  V = (np.linalg.norm(ry - a, axis=1) * np.linalg.norm(ry + a, axis=1) / 2) ** 2
  want = (-2 / beta * np.log(np.exp(V.reshape(100, 1000) * -beta / 2).mean(axis=1))).mean()
  print(f"[cost_rwpo] {res['true_val']:.12g} vs numpy {want:.12g}; evaluate: {res}")
  assert _rel(res["true_val"], want) <= 1e-10
  assert _rel(res["rel_err_pct"], (res["total"] - want) / want * 100) <= 1e-8
  assert abs(app.rwpo_true_value(2, 1, 1, 0.0, "quadratic") - 3.3863) <= 5e-5
  assert app.rwpo_true_value(2, 1, 1, 0.0, "obstacle") is None
  # ot
  config = solvers.load_config(overrides={"general": {"type": "ot"}})
  res = solvers.evaluate(config, model, params, rng)
  more = float(utils.calc_kinetic_energy(model.apply.sample, params, rng, batch_size=65536, t_size=10000, dim=2))
  less = float(utils.calc_kinetic_energy(model.apply.sample, params, rng, batch_size=4096, t_size=1000, dim=2))
  assert _rel(res["kinetic_energy_more"], more) <= 1e-12 and _rel(res["kinetic_energy_less"], less) <= 1e-12
  assert all(isinstance(v, float) for k, v in res.items() if k != "param_count")
  # fp: the density errors against the float64 restatement of rmse_mc_loss_fn / rmse_grid_loss_fn
  config = solvers.load_config(overrides={"general": {"type": "fp"}, "fp": {"velocity_field_type": "ou"}})
  f = config["fp"]
  res = solvers.evaluate(config, model, params, rng)
  print(f"[evaluate fp] {res}")
  flow = ol.OracleFlow(__import__("oracle").OracleConfig(D=2), params.flat.cpu().double().numpy())
  n = 1000000
  z = model.terms_backend(params).normal(rng, n).cpu().double().numpy()
  yy, lp = flow.sample_and_log_prob(z, [1.0])
  pf = np.exp(lp)
  for key, v0 in (("l2_mc", 4.0), ("l2_mc_ic", (f["T"] + 1) / 2)):
    want, sc = _want(pf, _mix64(yy, 1.0, v0, f["a"], f["T"]))
    _check(key, res[key] ** 2 * n, want, sc)
  xg = app.density_grid(500, -5.0, 5.0, range(500), dev).cpu().double().numpy()
  want, sc = _want(np.exp(flow.log_prob(xg, [1.0])), _mix64(xg, 1.0, 4.0, f["a"], f["T"]))
  _check("l2_grid", res["l2_grid"] ** 2 * 250000, want, sc)
  assert res["var_T_closed_form"] == app.ou_variance(f["T"], f["a"], (f["T"] + 1) / 2, f["sigma"])
  assert len(res["var_T"]) == 2


def _train(overrides, epochs):
  from cnf_ot_amd import solvers
  config = solvers.load_config(overrides=overrides)
  model, params, hist = solvers.train(config, epochs=epochs, capture=True)
  return config, model, params, hist


# Closed-form pins of trained runs (the default network, the captured step, the reference's 30 000 epochs; ~5 s each
# on the MI355X).  Observed values are in each test's docstring; each bound is about twice the observed value, the
# variance's capped at 5 %.
RWPO_REL_ERR_PCT_BOUND = 1.8
FP_VAR_BOUND = 0.05
FP_L2_IC_BOUND = 0.008


def test_trained_rwpo_quadratic_matches_its_closed_form(dev):
  """Config 3's problem: rwpo, quadratic potential, dim 2, T = 1, beta = 1, batch 2 048, 30 000 epochs: the
  evaluated total energy against dim (1 + log(T + 1)) / beta = 3.3863 (solvers.py:170-172).  Observed: total 3.4154
  (e_kin 1.3176, e_pot 2.0978), rel_err_pct 0.86."""
  import time
  from cnf_ot_amd import solvers
  t0 = time.time()
  config, model, params, hist = _train({"rwpo": {"T": 1, "beta": 1, "a": 0, "pot_type": "quadratic"},
                                        "train": {"batch_size": 2048}}, 30000)
  res = solvers.evaluate(config, model, params, 7)
  print(f"[pin rwpo quadratic] {res} ({time.time() - t0:.1f} s)")
  assert abs(res["true_val"] - 3.3863) <= 5e-5
  assert abs(res["rel_err_pct"]) <= RWPO_REL_ERR_PCT_BOUND


def test_trained_fp_ou_matches_its_closed_form_variance(dev):
  """fp with the OU drift, dim 2, a = 1, sigma = 0.5, T = 1, 30 000 epochs: the per-dimension variance at t = T
  against ou_variance(T, a, (T+1)/2, sigma), and the density error against the training's own initial condition.
  Observed: var_T 0.5829 / 0.5806 against 0.5677 (+2.7 % / +2.3 %: twice that would pass the 5 % ceiling, which is
  the bound), l2_mc_ic 0.0038 (l2_mc against the reference's variance-4 mixture: 0.051)."""
  import time
  from cnf_ot_amd import solvers
  t0 = time.time()
  config, model, params, hist = _train({"general": {"type": "fp"},
                                        "fp": {"T": 1, "a": 1, "sigma": 0.5, "velocity_field_type": "ou"}}, 30000)
  res = solvers.evaluate(config, model, params, 7)
  print(f"[pin fp ou] {res} ({time.time() - t0:.1f} s)")
  for v in res["var_T"]:
    assert abs(v / res["var_T_closed_form"] - 1) <= FP_VAR_BOUND
  assert res["l2_mc_ic"] <= FP_L2_IC_BOUND
