"""Fused importance-sampling diagnostics on the GPU: cnf_importance_stats(_seeded) / FlowEngine.importance_stats /
applications.importance_stats / solvers.evaluate_fit, against the float64 oracle (tests/importance_ref.py), with the
composition the engine offered before -- eng.sample_logprob's fp32 outputs pushed through the helper's float64
arithmetic -- as the yardstick for the fused kernel's error.  Measured values are printed.

Measured on one MI355X, fused / composed error against the oracle (max over the three times) and the largest
|log-weight| that enters the bound 2 e_composed + 1e-5 + 4 * 2^-23 * max|l| (four times it for log ess):
  D=2  8-mode mixture      log Z 4.84e-07 / 4.19e-07   KL 8.08e-07 / 5.15e-07   log ess 2.15e-06 / 1.45e-06   max|l| 4.7
  D=3  N(-3 1, A + I)      log Z 5.44e-06 / 5.35e-06   KL 6.73e-06 / 6.65e-06   log ess 2.02e-06 / 2.20e-06   max|l| 133.2
  D=10 N(0, 1.3 s I)       log Z 3.13e-06 / 2.19e-06   KL 2.08e-06 / 2.33e-06   log ess 3.43e-06 / 3.15e-06   max|l| 21.5
  D=14 N(0, I)             log Z 3.55e-06 / 2.78e-06   KL 4.21e-06 / 3.94e-06   log ess 4.19e-06 / 3.60e-06   max|l| 21.1
The eight compiled shapes at D=2: log Z 6.1e-08 .. 1.3e-06 fused against 3.8e-08 .. 1.4e-06 composed.  Underflow case
(identity flow, N(40 1, I), max|l| 1792): log Z -1406.192676, fused error 0 / composed 3.8e-07, ess 1.5630 = the
reference's.  Identity flow against itself: log Z 1.4e-08 / 6.8e-08, KL 6e-15 / 2.7e-14, ess/n - 1 -1e-14 / -5e-14 at
dim 2 / 10.
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CONDS = np.array([0.0, 0.35, 1.0], dtype=np.float32)
B_ORACLE = 700          # no multiple of 64 or 256: three tiles per slice, the last one 188 samples
A_SOURCE = np.array([[5.0, 1.0], [1.0, 0.5]])


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def _f32(x):
  return float(np.float32(x))


def _engine(dev, D, scale=0.2, seed=1, flat=None, **cfg_kw):
  from cnf_ot_amd import FlowConfig, FlowEngine, Params
  cfg = FlowConfig(dim=D, **cfg_kw)
  if flat is None:
    params = Params.zeros(cfg, dev) if scale == 0 else Params.random(cfg, scale, seed=seed, device=dev)
  else:
    params = Params(cfg, torch.from_numpy(flat).to(dev))
  return cfg, params, FlowEngine(cfg, dev).load(params)


def _ocfg(cfg):
  import oracle
  # (the C ABI carries the spline constants as float32: the oracle gets the same rounded values)
  return oracle.OracleConfig(D=cfg.dim, L=cfg.num_layers, H=cfg.hidden_size, M=cfg.mlp_num_layers, K=cfg.num_bins,
                             min_bin_size=_f32(cfg.min_bin_size), min_knot_slope=_f32(cfg.min_knot_slope))


def _targets(D):
  from cnf_ot_amd.applications import GaussianMixtureTarget, MIXTURE_CENTERS
  if D == 2:
    return GaussianMixtureTarget(MIXTURE_CENTERS.astype(np.float64)), None
  if D == 3:
    A = np.eye(3)
    A[:2, :2] = A_SOURCE
    return GaussianMixtureTarget([[-3.0] * 3], A), None
  if D == 10:
    return GaussianMixtureTarget(np.zeros((1, 10)), 1.3), [1.0, 0.8, 1.4]
  return GaussianMixtureTarget(np.zeros((1, D))), None


def _summaries(lw_slices):
  import importance_ref as ir
  return [ir.summary(lw) for lw in lw_slices]


def _errors(got_raw, ref):
  """max over slices of |log Z - ref|, |KL - ref|, |log ess - ref| of a raw [S, 5] block against reference summaries"""
  import importance_ref as ir
  got = [ir.summary_of_raw(r) for r in got_raw]
  return tuple(max(abs(f(g[k]) - f(r[k])) for g, r in zip(got, ref))
               for k, f in (("log_Z", float), ("KL", float), ("ess", math.log)))


def _check_against_oracle(dev, eng, cfg, flat64, tg, scales, tag):
  """The issue's bound: e_fused <= 2 e_composed + 1e-5 + 4 * 2^-23 * max|l| for log Z and KL, four times it for log ess"""
  import importance_ref as ir
  import oracle
  S, B = len(CONDS), B_ORACLE
  noise = eng.normal(500 + cfg.dim, S * B)
  raw = eng.importance_stats(tg, noise, CONDS, scale=scales)
  assert eng.last_path() == "importance" and raw.shape == (S, 5) and raw.dtype == torch.float64
  y32, lp32 = eng.sample_logprob(noise, torch.from_numpy(CONDS).to(dev))
  torch.cuda.synchronize()
  raw = raw.cpu().numpy()
  assert np.array_equal(raw[:, 4], [B] * S)
  ref_parts = ir.oracle_log_weights(oracle, _ocfg(cfg), flat64, noise.cpu().double().numpy(), CONDS, tg, scales)
  ref = _summaries([p[0] for p in ref_parts])
  y, lp = y32.cpu().double().numpy(), lp32.cpu().double().numpy()
  comp_lw = [ir.log_weights(tg, y[s * B:(s + 1) * B], lp[s * B:(s + 1) * B], 1.0 if scales is None else scales[s])
             for s in range(S)]
  e_comp = _errors(np.stack([ir.raw_state(lw) for lw in comp_lw]), ref)
  e_fused = _errors(raw, ref)
  max_l = max(np.abs(p[0]).max() for p in ref_parts)
  slack = 1e-5 + 4.0 * 2.0 ** -23 * max_l
  print(f"\n[importance {tag}] log Z {e_fused[0]:.2e} / {e_comp[0]:.2e}  KL {e_fused[1]:.2e} / {e_comp[1]:.2e}  "
        f"log ess {e_fused[2]:.2e} / {e_comp[2]:.2e}  (fused / composed; max|l| {max_l:.1f}, slack {slack:.2e}; "
        f"log Z {[round(float(r['log_Z']), 4) for r in ref]}, ess {[round(float(r['ess']), 1) for r in ref]})")
  assert e_fused[0] <= 2 * e_comp[0] + slack
  assert e_fused[1] <= 2 * e_comp[1] + slack
  assert e_fused[2] <= 4 * (2 * e_comp[2] + slack)


# 1 ---- against the float64 oracle
@pytest.mark.parametrize("D,scale", [(2, 0.2), (3, 0.15), (10, 0.12), (14, 0.1)])
def test_against_the_float64_oracle(dev, oracle_lib, D, scale):
  cfg, params, eng = _engine(dev, D, scale, seed=100 + D)
  tg, scales = _targets(D)
  _check_against_oracle(dev, eng, cfg, params.flat.cpu().double().numpy(), tg, scales, f"D={D}")


# 2 ---- shapes: tails, one wave, one tile + 1, two tiles + 1, several chunks per slice
@pytest.mark.parametrize("B", [1, 63, 257, 513, 3000])
def test_shapes_shared_noise_and_slices_alone(dev, B):
  _, _, eng = _engine(dev, 2, 0.2, seed=5)
  tg, _ = _targets(2)
  t = np.linspace(0.0, 1.0, 7).astype(np.float32)
  noise = eng.normal(21, B)
  shared = eng.importance_stats(tg, noise, t, shared=True)
  assert shared.shape == (7, 5) and torch.equal(shared[:, 4], torch.full((7,), float(B), dtype=torch.float64, device=dev))
  assert torch.isfinite(shared).all()
  repeated = eng.importance_stats(tg, noise.repeat(7, 1), t)
  assert torch.equal(shared, repeated)
  for s in range(7):
    alone = eng.importance_stats(tg, noise, t[s:s + 1])
    assert torch.equal(alone[0], shared[s]), (B, s)
  assert not torch.equal(shared[0], shared[6])


# 3 ---- seeded == given
@pytest.mark.parametrize("D,B,stride", [(2, 700, 700), (2, 700, 0), (3, 301, 1000), (3, 301, 0)])
def test_seeded_equals_fill_normal_then_given(dev, D, B, stride):
  _, _, eng = _engine(dev, D, 0.15, seed=6)
  tg, _ = _targets(D)
  seed, first = 1234, 37
  if stride == 0:
    given = eng.importance_stats(tg, eng.normal(seed, B, first_sample=first), CONDS, shared=True)
  else:
    noise = torch.cat([eng.normal(seed, B, first_sample=first + s * stride) for s in range(3)])
    given = eng.importance_stats(tg, noise, CONDS)
  seeded = eng.importance_stats(tg, t=CONDS, B=B, seed=seed, first_sample=first, slice_stride=stride)
  assert torch.equal(seeded, given)


# 4 ---- reproducible
def test_two_calls_are_bit_identical(dev):
  _, _, eng = _engine(dev, 10, 0.12, seed=8)
  tg, scales = _targets(10)
  a = eng.importance_stats(tg, t=CONDS, B=5000, seed=3, scale=scales)
  b = eng.importance_stats(tg, t=CONDS, B=5000, seed=3, scale=scales)
  assert torch.equal(a, b) and torch.isfinite(a).all()


# 5 ---- where the reference's linear-space formula gives Z = 0 and ESS = NaN
def test_underflow_on_the_device(dev, oracle_lib):
  import importance_ref as ir
  import oracle
  from cnf_ot_amd.applications import GaussianMixtureTarget, importance_summary
  cfg, params, eng = _engine(dev, 2, 0)
  tg = GaussianMixtureTarget([[40.0, 40.0]])
  B = 4096
  noise = eng.normal(3, B)
  raw = eng.importance_stats(tg, noise, [0.5])
  y32, lp32 = eng.sample_logprob(noise, 0.5)
  got = {k: float(v[0]) for k, v in importance_summary(raw.cpu()).items() if k != "raw"}
  (lw, y_ref, lq_ref), = ir.oracle_log_weights(oracle, _ocfg(cfg), np.zeros(cfg.param_count()), noise.cpu().double().numpy(),
                                               [0.5], tg)
  ref = ir.summary(lw)
  nv = ir.naive(lw + lq_ref, lq_ref)
  assert nv["Z"] == 0.0 and not np.isfinite(nv["ess"])
  comp = ir.summary(ir.log_weights(tg, y32.cpu().double().numpy(), lp32.cpu().double().numpy()))
  slack = 1e-5 + 4.0 * 2.0 ** -23 * np.abs(lw).max()
  e_f, e_c = abs(got["log_Z"] - ref["log_Z"]), abs(comp["log_Z"] - ref["log_Z"])
  print(f"\n[importance underflow] log Z {got['log_Z']:.6f} (ref {ref['log_Z']:.6f}; fused {e_f:.2e} / composed {e_c:.2e}, "
        f"slack {slack:.2e})  ess {got['ess']:.4f} (ref {ref['ess']:.4f})  max|l| {np.abs(lw).max():.1f}")
  assert math.isfinite(got["log_Z"]) and e_f <= 2 * e_c + slack
  assert 1.0 < got["ess"] <= B


# 6 ---- identity flow against its own base density
@pytest.mark.parametrize("D", [2, 10])
def test_identity_flow_against_itself(dev, D):
  from cnf_ot_amd.applications import GaussianMixtureTarget, importance_summary
  _, _, eng = _engine(dev, D, 0)
  n = 20000
  s = importance_summary(eng.importance_stats(GaussianMixtureTarget(np.zeros((1, D))), t=[0.0, 1.0], B=n, seed=2).cpu())
  print(f"\n[importance identity D={D}] log Z {s['log_Z'].tolist()}  KL {s['KL'].tolist()}  ess/n - 1 {(s['ess'] / n - 1).tolist()}")
  assert s["log_Z"].abs().max() <= 1e-6 and s["KL"].abs().max() <= 1e-6 and (s["ess"] / n - 1).abs().max() <= 1e-6
  assert s["ess_pct"].sub(100).abs().max() <= 1e-4 and s["n"].tolist() == [n, n]


# 7 ---- nothing is hidden
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_non_finite_sample_poisons_its_slice_alone(dev, bad):
  _, _, eng = _engine(dev, 3, 0.15, seed=9)
  tg, _ = _targets(3)
  B = 700
  noise = eng.normal(4, 3 * B)
  clean = eng.importance_stats(tg, noise, CONDS)
  dirty_noise = noise.clone()
  dirty_noise[B + 300, 1] = bad
  dirty = eng.importance_stats(tg, dirty_noise, CONDS)
  assert torch.isnan(dirty[1, :4]).all() and float(dirty[1, 4]) == B
  assert torch.equal(dirty[0], clean[0]) and torch.equal(dirty[2], clean[2]) and torch.isfinite(clean).all()


# 8 ---- argument errors: the code, and nothing written
def test_argument_errors_leave_stats_untouched(dev):
  from cnf_ot_amd import FlowConfig, FlowEngine, Params, _capi
  from cnf_ot_amd.flows import _stream_ptr
  cfg, params, eng = _engine(dev, 2, 0.2)
  tg, _ = _targets(2)
  S, B = 3, 700
  noise = eng.normal(1, S * B)
  t = torch.from_numpy(CONDS).to(dev)
  stats = torch.full((S, 5), -7.0, dtype=torch.float64, device=dev)
  nbytes = ctypes.c_int64(0)
  assert eng.lib.cnf_importance_workspace(S, B, 2, ctypes.byref(nbytes)) == _capi.CNF_OK
  work = torch.empty(nbytes.value // 8, dtype=torch.float64, device=dev)

  def call(h=None, spec=None, noise_p=noise.data_ptr(), t_p=t.data_ptr(), n_slices=S, b=B, stats_p=stats.data_ptr(),
           work_p=work.data_ptr(), wbytes=nbytes.value, seeded=None):
    h = eng._h if h is None else (None if h == "null" else h)
    spec = ctypes.byref(tg.spec) if spec is None else spec
    if seeded is not None:
      return eng.lib.cnf_importance_stats_seeded(h, spec, 5, seeded[0], seeded[1], t_p, n_slices, b, stats_p, work_p, wbytes,
                                                 _stream_ptr(dev))
    return eng.lib.cnf_importance_stats(h, spec, noise_p, 0, t_p, n_slices, b, stats_p, work_p, wbytes, _stream_ptr(dev))

  def variant(**kw):
    s = _capi.CnfTargetSpec.from_buffer_copy(tg.spec)
    for k, v in kw.items():
      if k == "diag":
        s.W[v[0]][v[0]] = v[1]
      else:
        setattr(s, k, v)
    return ctypes.byref(s)

  invalid = [dict(h="null"), dict(h="null", seeded=(0, B)), dict(spec=ctypes.POINTER(_capi.CnfTargetSpec)()), dict(noise_p=None), dict(t_p=None), dict(stats_p=None),
             dict(work_p=None), dict(n_slices=-1), dict(b=-1), dict(seeded=(-1, B)), dict(seeded=(0, -1)),
             dict(spec=variant(n_comp=0)), dict(spec=variant(n_comp=9)), dict(spec=variant(diag=(1, 0.0))),
             dict(spec=variant(diag=(0, -1.0))), dict(spec=variant(diag=(1, float("nan")))),
             dict(spec=variant(diag=(0, float("inf")))), dict(wbytes=nbytes.value - 1), dict(wbytes=0), dict(wbytes=-1)]
  for kw in invalid:
    assert call(**kw) == _capi.CNF_ERR_INVALID, kw
  unset = FlowEngine(cfg, dev)                                   # parameters never set
  assert call(h=unset._h) == _capi.CNF_ERR_INVALID
  tcfg = FlowConfig.torus(dim=2)
  torus = FlowEngine(tcfg, dev).load(Params.random(tcfg, 0.2, seed=1, device=dev))
  assert call(h=torus._h) == _capi.CNF_ERR_UNSUPPORTED
  # nothing to do: OK, nothing launched
  assert call(n_slices=0) == _capi.CNF_OK and call(b=0) == _capi.CNF_OK
  torch.cuda.synchronize()
  assert torch.equal(stats, torch.full((S, 5), -7.0, dtype=torch.float64, device=dev))
  # ... and the same buffers in a valid call are written
  assert call() == _capi.CNF_OK
  torch.cuda.synchronize()
  assert torch.equal(stats, eng.importance_stats(tg, noise, CONDS))
  # the tensor wrapper: the empty state for an empty batch, its own argument checks
  empty = eng.importance_stats(tg, t=CONDS, B=0, seed=1)
  assert torch.equal(empty[:, 0], torch.full((3,), -math.inf, dtype=torch.float64, device=dev)) and not empty[:, 1:].any()
  with pytest.raises(ValueError):
    eng.importance_stats(tg, noise, CONDS, seed=1)
  with pytest.raises(ValueError):
    eng.importance_stats(tg, noise[:-1], CONDS)
  with pytest.raises(ValueError):
    eng.importance_stats(tg, noise, CONDS, scale=[1.0, 2.0])


# 9 ---- every compiled shape
def _shape_ids():
  from network_shapes import kernel_configs
  return [pytest.param(h, k, id=f"h{h}k{k}") for h, k in kernel_configs()]


@pytest.mark.parametrize("H,K", _shape_ids())
def test_every_compiled_shape(dev, oracle_lib, H, K):
  from network_shapes import param_scale
  s = param_scale(H, 2, 2)
  cfg, params, eng = _engine(dev, 2, s, seed=H * 10 + K, hidden_size=H, num_bins=K)
  tg, _ = _targets(2)
  _check_against_oracle(dev, eng, cfg, params.flat.cpu().double().numpy(), tg, None, f"h{H}k{K} s={s}")


# 10 ---- sharded == whole
def test_applications_shards_merge_to_the_whole(dev):
  from cnf_ot_amd import FlowConfig, FlowModel, Params
  from cnf_ot_amd import applications as app
  from cnf_ot_amd.distributed import Shard
  cfg = FlowConfig(dim=3)
  model = FlowModel(cfg)
  params = Params.random(cfg, 0.15, seed=4, device=dev)
  tg, _ = _targets(3)
  n = 10001          # odd: the two ranks' blocks differ in length
  whole = app.importance_stats(model, params, tg, CONDS, 77, n)
  parts = [app.importance_stats(model, params, tg, CONDS, 77, n, shard=Shard(r, 2)) for r in (0, 1)]
  assert [int(p["n"][0]) for p in parts] == [5001, 5000] and whole["n"].tolist() == [n] * 3
  merged = app.importance_summary(app.merge_importance_stats([p["raw"] for p in parts]))
  assert torch.equal(merged["max_log_w"], whole["max_log_w"]) and torch.equal(merged["n"], whole["n"])
  for k in ("log_Z", "KL", "ess", "ess_pct"):
    rel = ((merged[k] - whole[k]).abs() / whole[k].abs().clamp_min(1e-300)).max()
    assert float(rel) <= 1e-12, (k, float(rel))
  rel = ((merged["raw"] - whole["raw"]).abs() / whole["raw"].abs()).max()
  assert float(rel) <= 1e-12
  with pytest.raises(ValueError):
    app.importance_stats(model, params, _targets(2)[0], CONDS, 77, n)


# 11 ---- the evaluation entry point
def test_evaluate_fit_on_the_untrained_ot_flow(dev, capsys):
  from cnf_ot_amd import Params, solvers
  config = solvers.load_config(overrides={"general": {"type": "ot"}})
  model = solvers.build_model(config)
  params = Params.zeros(model.cfg, dev)
  res = solvers.evaluate_fit(config, model, params, 11, batch_size=1 << 16)
  assert res["times"] == [0.0, 1.0] and res["batch_size"] == 1 << 16
  for k in ("log_Z", "KL", "ess", "ess_pct", "max_log_w"):
    assert len(res[k]) == 2 and all(math.isfinite(v) for v in res[k]), (k, res[k])
  print(f"\n[evaluate_fit] {res}")
  assert abs(res["ess_pct"][1] - 100.0) <= 1e-4          # the identity flow IS the target at T
  capsys.readouterr()
  solvers.print_fit(res)
  assert capsys.readouterr().out.count("\n") == 3
