"""GPU parity of the backward pass (cnf_loss_terms_grad) and of the Adam update.

Reference gradients: central finite differences (float64) of the oracle's
restatement of each loss term over ALL parameters -- what
`jax.value_and_grad(loss_fn)` of cnf_ot/mfc/solvers.py:94 differentiates.
The losses are piecewise smooth in the parameters (ReLU, bin boundaries), and
the finite-difference-in-time terms weight a sample whose ReLU switches between
t - dt/2 and t + dt/2 by 1/dt, so a difference quotient that straddles such a
kink is off by O(1): the reference is taken at h = 1e-7 and entries where
h = 1e-6 disagrees are excluded (and counted) instead of being compared.

Tolerance: |g_gpu - g_fd|_inf <= 5e-3 * |g_fd|_inf for the finite-difference
terms (their per-sample velocities are fp32 differences divided by dt = 0.01,
and the gradient is a difference of two such Jacobian products), 1e-3 for the
direct terms.  Measured values are printed.
Every parameter of every tensor, at more shapes and at float32-noise bounds: test_gpu_flow_adjoint.py (analytic float64 adjoint).
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def _fd_grad(fn, params64, idx):
  """(reference gradient at h = 1e-7 on the entries `idx`, mask of entries where h = 1e-6 agrees)."""
  out = []
  for h in (1e-7, 1e-6):
    g = np.zeros_like(params64)
    for i in idx:
      p = params64.copy(); p[i] += h
      fp = fn(p)
      p[i] -= 2 * h
      g[i] = (fp - fn(p)) / (2 * h)
    out.append(g)
  scale = max(np.abs(out[0]).max(), 1e-30)
  ok = np.zeros(params64.size, dtype=bool)
  ok[idx] = (np.abs(out[0] - out[1]) <= 1e-5 * scale)[idx]
  return out[0], ok


def _run(dev, D, kind_spec, B, n_slices, shared, scale_params, seed, rtol, name, spread=1.5):
  from oracle_backend import OracleBackend
  from cnf_ot_amd import FlowConfig, FlowEngine, Params
  cfg = FlowConfig(dim=D)
  params = Params.random(cfg, scale_params, seed=seed, device=dev)
  eng = FlowEngine(cfg, dev).load(params)
  pts = eng.normal(seed + 1, B if shared else B * n_slices)
  if kind_spec.kind == 5:            # NEG_LOGPROB: data points, not base noise
    pts = pts * spread + 0.3
  t = np.linspace(0.2, 0.8, n_slices).astype(np.float32)
  grad = torch.zeros(cfg.param_count(), device=dev)
  sums = eng.loss_terms_grad(kind_spec, pts, t, B, shared, 1.0, grad)
  sums_fwd = eng.loss_terms(kind_spec, pts, t, B, shared)
  # the gradient kernel evaluates the conditioner on the matrix cores, the loss kernel on the vector ALU: two fp32
  # evaluation orders.  The finite-difference terms amplify the difference by 1/dt and 1/dx = 100.
  fd_term = kind_spec.kind <= 2
  assert torch.allclose(sums, sums_fwd, rtol=5e-5 if fd_term else 2e-6, atol=1e-6), (sums, sums_fwd)
  # a second call accumulates and is deterministic
  grad2 = torch.zeros_like(grad)
  eng.loss_terms_grad(kind_spec, pts, t, B, shared, 1.0, grad2)
  assert torch.equal(grad, grad2)
  pts64 = pts.cpu()
  p64 = params.flat.cpu().double().numpy()
  f = lambda p: float(OracleBackend(cfg, p).loss_terms(kind_spec, pts64, t, B, shared).sum())
  # the 16 parameters of the shared `first` spline + a random 15 % of the conditioner weights
  # (every tensor of every conditioner is hit; the full set takes minutes of CPU oracle time)
  rs = np.random.default_rng(seed)
  idx = np.concatenate([np.arange(16), 16 + rs.choice(p64.size - 16, max(1, (p64.size - 16) * 15 // 100), replace=False)]) \
    if p64.size > 16 else np.arange(p64.size)
  g_fd, smooth = _fd_grad(f, p64, idx)
  g = grad.cpu().double().numpy()
  n_kink = int(idx.size - smooth.sum())
  err = np.abs(g - g_fd)[smooth].max() / max(np.abs(g_fd).max(), 1e-30)
  first_err = np.abs(g[:16] - g_fd[:16]).max() / max(np.abs(g_fd[:16]).max(), 1e-30)
  print(f"[grad {name} D={D}] |g|inf={np.abs(g_fd).max():.4g} rel err={err:.2e} (first-spline block {first_err:.2e}; "
        f"{n_kink} of {idx.size} checked entries at a kink excluded)")
  assert n_kink <= 0.02 * idx.size + 1
  assert err <= rtol, (name, err)
  return g, g_fd


def _spec(kind, **kw):
  from cnf_ot_amd.applications import _spec as mk
  return mk(kind, **kw)


def test_grad_direct_terms(dev):
  from cnf_ot_amd import _capi
  _run(dev, 2, _spec(_capi.TERM_NEG_LOGPROB), 200, 1, True, 0.2, 3, 1e-3, "neg_logprob")
  for sub in (0, 1, 2):
    _run(dev, 2, _spec(_capi.TERM_POTENTIAL, subtype=sub, a=1.0), 200, 2, True, 0.2, 4 + sub, 1e-3, f"potential{sub}")
  _run(dev, 2, _spec(_capi.TERM_REVERSE_KL, T=1.0, beta=4.0), 300, 1, True, 0.2, 8, 1e-3, "reverse_kl")


def test_grad_with_points_on_the_linear_tails(dev):
  """The density-fit term's parameter gradient with a quarter of the points beyond the splines' range (|x| > 10):
  the tails' slopes are conditioner outputs, so the weight gradient sees them (and saw the upper tail wrongly before
  `BinPartials::f_y0`)."""
  from cnf_ot_amd import _capi
  _run(dev, 2, _spec(_capi.TERM_NEG_LOGPROB), 300, 1, True, 0.2, 31, 1e-3, "neg_logprob_tails", spread=7.0)
  _run(dev, 3, _spec(_capi.TERM_NEG_LOGPROB), 200, 1, True, 0.15, 32, 1e-3, "neg_logprob_tails_d3", spread=7.0)


def test_grad_finite_difference_terms(dev):
  from cnf_ot_amd import _capi
  _run(dev, 2, _spec(_capi.TERM_KINETIC, dt=0.01), 200, 2, False, 0.2, 9, 5e-3, "kinetic")
  _run(dev, 2, _spec(_capi.TERM_KINETIC_SCORE, dt=0.01, dx=0.01, coef=0.5), 200, 1, True, 0.2, 10, 5e-3, "kinetic_score")
  for sub in (0, 1, 2):
    _run(dev, 2, _spec(_capi.TERM_FLOW_MATCHING, subtype=sub, dt=0.01, dx=0.01, coef=0.5, a=1.0), 128, 1, True, 0.2,
         11 + sub, 5e-3, f"flow_matching{sub}")


def test_grad_other_dims(dev):
  from cnf_ot_amd import _capi
  _run(dev, 1, _spec(_capi.TERM_NEG_LOGPROB), 100, 1, True, 0.4, 20, 1e-3, "neg_logprob")
  _run(dev, 3, _spec(_capi.TERM_FLOW_MATCHING, subtype=3, dt=0.01, dx=0.01, coef=0.5, a=1.0), 64, 1, True, 0.15, 21,
       5e-3, "flow_matching_lorenz")
  _run(dev, 3, _spec(_capi.TERM_REVERSE_KL, T=1.0, beta=4.0), 100, 1, True, 0.15, 22, 1e-3, "reverse_kl")


@pytest.mark.parametrize("D", [4, 7, 10, 13])
def test_grad_higher_dims_against_the_oracle(dev, D):
  """The matrix-core conditioner of the backward kernels at every first-layer shape: 1 + d inputs + the bias row are
  ceil((d + 2) / 4) MFMA k-steps (2 at dim 4, up to 4 at dim 13), the same rows are the A operand of the first
  layer's weight-gradient GEMM and the rows of W0 g1 its input adjoints.  Against central differences of the float64
  oracle over the `first` block and a random subset of the conditioner weights: the fused loss kernel (generic
  dimension: no look-ahead, `first` accumulators in LDS) on a data -> base and a base -> data term, and cnf_pass_vjp
  (the look-ahead kernel) in both directions, parameter gradient and input adjoints."""
  import oracle
  from cnf_ot_amd import FlowConfig, FlowEngine, Params, _capi
  sc = 0.25 / np.sqrt(D)
  _run(dev, D, _spec(_capi.TERM_NEG_LOGPROB), 96, 2, False, sc, 30 + D, 2e-3, "neg_logprob")
  _run(dev, D, _spec(_capi.TERM_REVERSE_KL, T=1.0, beta=4.0), 96, 1, True, sc, 40 + D, 2e-3, "reverse_kl")
  cfg = FlowConfig(dim=D); ocfg = oracle.OracleConfig(D=D)
  params = Params.random(cfg, sc, seed=50 + D, device=dev)
  eng = FlowEngine(cfg, dev).load(params)
  B = 200
  gen = torch.Generator(device="cpu").manual_seed(D)
  pts = (torch.randn(B, D, generator=gen) * 1.3).to(dev)
  ybar = torch.randn(B, D, generator=gen).to(dev)
  ldbar = torch.randn(B, generator=gen).to(dev)
  c = torch.rand(B, generator=gen).to(dev)
  p64 = params.flat.cpu().double().numpy()
  x64, yb, lb, c64 = pts.cpu().double().numpy(), ybar.cpu().double().numpy(), ldbar.cpu().double().numpy(), c.cpu().double().numpy()
  rs = np.random.default_rng(D)
  idx = np.concatenate([np.arange(16), 16 + rs.choice(p64.size - 16, 400, replace=False)])
  for to_base in (False, True):
    fn = oracle.inverse_logdet if to_base else oracle.forward_logdet

    def scalar(p, x=x64):
      y, ld = fn(ocfg, p, x, c64)
      return float((y * yb).sum() + (ld * lb).sum())

    g = torch.zeros(cfg.param_count(), device=dev)
    xb = eng.pass_vjp(pts, c[:, None], ybar, ldbar, to_base, grad=g)
    g_fd, smooth = _fd_grad(scalar, p64, idx)
    gg = g.cpu().double().numpy()
    err = np.abs(gg - g_fd)[smooth].max() / np.abs(g_fd).max()
    # input adjoints: central differences in x, one coordinate of every point at a time
    xb_fd = np.zeros((B, D)); h = 1e-6
    for e in range(D):
      xp = x64.copy(); xm = x64.copy(); xp[:, e] += h; xm[:, e] -= h
      yp, lp = fn(ocfg, p64, xp, c64); ym, lm = fn(ocfg, p64, xm, c64)
      xb_fd[:, e] = (((yp - ym) * yb).sum(1) + (lp - lm) * lb) / (2 * h)
    ex = np.abs(xb.cpu().double().numpy() - xb_fd).max() / np.abs(xb_fd).max()
    print(f"[pass_vjp D={D} to_base={to_base}] grad rel {err:.2e} ({int(idx.size - smooth.sum())} kink entries)  xbar rel {ex:.2e}")
    assert err <= 2e-3 and ex <= 2e-3 and idx.size - smooth.sum() <= 0.03 * idx.size + 1


def test_value_and_grad_of_composite_losses(dev):
  """applications.value_and_grad over ot / rwpo / fp losses == finite differences
  of the same composition over the float64 oracle (a random subset of the
  parameters, kink-robust reference as above)."""
  from functools import partial
  from oracle_backend import OracleModel
  from cnf_ot_amd import FlowConfig, FlowModel, Params
  from cnf_ot_amd import applications as app
  from cnf_ot_amd.distributed import Shard
  cfg = FlowConfig(dim=2)
  model, omodel = FlowModel(cfg), OracleModel(cfg)
  params = Params.random(cfg, 0.2, seed=31, device=dev)
  B, seed = 256, 5
  cases = {
    "ot_obstacle": (partial(app.ot_loss_fn, model, 2, 1.0, 0.01, 2, "obstacle"), partial(app.ot_loss_fn, omodel, 2, 1.0, 0.01, 2, "obstacle")),
    "rwpo_double_well": (partial(app.rwpo_loss_fn, model, 2, 2.0, 10.0, 0.01, 0.01, 2, "double_well", 1.0),
                         partial(app.rwpo_loss_fn, omodel, 2, 2.0, 10.0, 0.01, 0.01, 2, "double_well", 1.0)),
    "fp_gradient": (partial(app.fp_loss_fn, model, 2, 1.0, 1.0, 0.5, 0.01, 0.01, 2, "gradient"),
                    partial(app.fp_loss_fn, omodel, 2, 1.0, 1.0, 0.5, 0.01, 0.01, 2, "gradient")),
  }
  rng = np.random.default_rng(0)
  idx = np.concatenate([np.arange(16), rng.choice(np.arange(16, cfg.param_count()), 64, replace=False)])
  for name, (gpu_fn, ora_fn) in cases.items():
    loss, grads = app.value_and_grad(gpu_fn)(params, seed, 5000.0, B)
    loss_plain = gpu_fn(params, seed, 5000.0, B)
    assert abs(float(loss) - float(loss_plain)) <= 1e-6 * abs(float(loss_plain))
    assert set(grads.keys()) == set(params.keys())                      # haiku tree
    g = grads.flat.cpu().double().numpy()
    cpu = Params(cfg, params.flat.cpu().clone())      # only carries cfg: the oracle reads float64 `q`
    # float32 parameter storage cannot resolve h = 1e-7: differentiate the oracle composition in float64 directly
    from oracle_backend import OracleBackend
    p64 = params.flat.cpu().double().numpy()

    class _M:      # OracleModel over raw float64 parameters
      def __init__(self, q): self.q = q
      def terms_backend(self, _params, device=None): return OracleBackend(cfg, self.q)

    def loss_at(q):
      fn = ora_fn.func
      return float(fn(_M(q), *ora_fn.args[1:], cpu, seed, 5000.0, B, shard=Shard()))
    ref, ok = np.zeros(idx.size), np.zeros(idx.size, dtype=bool)
    for n, i in enumerate(idx):
      vals = []
      for h in (1e-7, 1e-6):
        q = p64.copy(); q[i] += h; fp = loss_at(q); q[i] -= 2 * h; vals.append((fp - loss_at(q)) / (2 * h))
      ref[n] = vals[0]; ok[n] = abs(vals[0] - vals[1]) <= 1e-5 * max(np.abs(g).max(), 1e-30)
    scale = max(np.abs(ref).max(), np.abs(g[idx]).max())
    err = np.abs(g[idx] - ref)[ok].max() / scale
    print(f"[value_and_grad {name}] loss={float(loss):.6g} |g|inf={scale:.4g} rel err={err:.2e} ({int((~ok).sum())} kink entries excluded)")
    assert err <= 5e-3 and (~ok).sum() <= 4


def test_adam_step_and_training_decreases_loss(dev):
  from cnf_ot_amd import solvers, FlowConfig, Params
  cfg = FlowConfig(dim=2)
  p = Params.random(cfg, 0.3, seed=1, device=dev)
  g = Params.random(cfg, 1.0, seed=2, device=dev)
  opt = solvers.Adam(1e-3)
  st = opt.init(p)
  p0 = p.flat.cpu().double().numpy().copy(); gg = g.flat.cpu().double().numpy()
  mu = np.zeros_like(p0); nu = np.zeros_like(p0); ref = p0.copy()
  for step in range(1, 4):       # optax.adam: bias-corrected moments, eps outside the sqrt
    st = opt.apply(p, g, st)
    mu = 0.9 * mu + 0.1 * gg; nu = 0.999 * nu + 0.001 * gg * gg
    ref -= 1e-3 * (mu / (1 - 0.9 ** step)) / (np.sqrt(nu / (1 - 0.999 ** step)) + 1e-8)
    assert np.abs(p.flat.cpu().double().numpy() - ref).max() <= 2e-6
  assert st.step == 3
  # a short OT run from the identity flow: the loss must go down (solvers.py:99-127 in miniature)
  config = solvers.load_config(overrides={"general": {"type": "ot", "t_batch_size": 2}, "train": {"batch_size": 2048, "lr": 1e-3}})
  model, params, hist = solvers.train(config, epochs=60)
  first, last = float(torch.stack(hist[:5]).mean()), float(torch.stack(hist[-5:]).mean())
  print(f"[train ot] loss {first:.5g} -> {last:.5g} after 60 Adam steps")
  assert np.isfinite(last) and last < first
  # the same loop with every step after the second replayed from ONE HIP graph (solvers.CapturedUpdate)
  model, params, hist = solvers.train(config, epochs=60, capture=True)
  first, last = float(torch.stack(hist[:5]).mean()), float(torch.stack(hist[-5:]).mean())
  print(f"[train ot, captured step] loss {first:.5g} -> {last:.5g} after 60 Adam steps")
  assert np.isfinite(last) and last < first


@pytest.mark.parametrize("kind", ["ot", "rwpo", "ot_large", "rwpo_dim6", "fp_dim6"])
def test_captured_step_equals_the_eager_step_bit_for_bit(dev, kind):
  """solvers.CapturedUpdate: `update` (solvers.py:90-97) captured into one HIP graph -- key, time batch, mixture
  components, base noise and Adam's step count all read from device memory -- against the very same body run
  eagerly: after 10 steps from the same start the parameters and both Adam moments are the same BITS, and every
  step's loss too."""
  from cnf_ot_amd import solvers
  B = 2048
  if kind == "ot_large":      # a batch whose terms run as the fused table-backward calls (cnf_neg_logprob_vjp, cnf_kinetic_potential_vjp)
    kind, B = "ot", 1 << 21
  ov = {"general": {"type": kind, "t_batch_size": 8 if B > 2048 else 2}, "train": {"batch_size": B, "lr": 1e-3}}
  if kind.endswith("_dim6"):      # the score terms from separate launches (applications._score_terms_unfused) inside the graph
    ov["general"].update(type=kind[:-5], dim=6)
    ov["fp"] = {"velocity_field_type": "ou"}
  config = solvers.load_config(overrides=ov)
  res = []
  for replay in (False, True):
    model = solvers.build_model(config)
    params = model.init(7)
    params.flat.add_(0.05 * torch.randn(params.flat.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1)))
    opt = solvers.Adam(1e-3); st = opt.init(params)
    upd = solvers.CapturedUpdate(solvers.bind_loss(config, model), opt, B, replay=replay)
    losses = []
    for step in range(10):
      loss, params, st = upd(params, 1000 + 17 * step, 5000.0, st)
      losses.append(loss.clone())
    torch.cuda.synchronize()
    assert (upd.graph is not None) == replay and st.step == 10
    res.append((params.flat.clone(), st.mu.clone(), st.nu.clone(), torch.stack(losses)))
  for a, b in zip(res[0], res[1]):
    assert torch.equal(a, b)
  assert torch.isfinite(res[0][3]).all() and res[0][3][0] != res[0][3][1]      # a new key (new draws) every step


def test_device_drawn_step_inputs_against_the_oracle(dev):
  """The draws of a captured step (cnf_fill_uniform_dev / cnf_mixture_source_dev / cnf_fill_normal_dev, keyed from
  device memory): read back and fed to the float64 restatement of applications.py -- the OT loss of a DeviceRng call
  is the oracle's loss on those very inputs; and the noise is the cnf_fill_normal stream of the same key."""
  import oracle
  from oracle import losses as ol
  from cnf_ot_amd import FlowConfig, FlowModel, Params, DeviceRng, applications as app, _capi
  from cnf_ot_amd.flows import _stream_ptr
  cfg = FlowConfig(dim=2); model = FlowModel(cfg)
  params = Params.random(cfg, 0.2, seed=4, device=dev)
  B, tbs, key = 4096, 3, 0x123456789ABCDEF1
  rng = DeviceRng(dev).set_key(key)
  tb = app.draw_t_batch(rng, tbs).cpu().numpy().astype(np.float64)
  assert tb.min() >= 0.0 and tb.max() < 1.0 and len(set(tb.tolist())) == tbs
  comp = torch.empty(B, dtype=torch.int32, device=dev)
  _capi.check(_capi.lib().cnf_mixture_source_dev(rng.ptr, 0, B, None, None, comp.data_ptr(), _stream_ptr(dev)), "comp")
  comp = comp.cpu().numpy().astype(np.int64)
  assert comp.min() == 0 and comp.max() == 7 and np.bincount(comp, minlength=8).min() > B / 8 * 0.7
  eng = model.terms_backend(params)
  assert torch.equal(eng.normal(rng, B), eng.normal(key, B))
  got = float(app.ot_loss_fn(model, 2, 1.0, 0.01, tbs, "free", params, rng, 5000.0, B, source="mixture"))
  flow = ol.OracleFlow(oracle.OracleConfig(D=2), params.flat.cpu().double().numpy())
  z = eng.normal(key, B).cpu().double().numpy()
  want = ol.ot_loss_fn(flow, 2, 1.0, 0.01, "free", 5000.0, B, z, tb, "mixture", comp)
  print(f"\n[device draws] ot loss {got:.8g} vs oracle {want:.8g}")
  assert abs(got - want) <= 2e-5 * abs(want)


def test_jacobian_helpers_match_finite_differences(dev):
  """forward_jac / inverse_jac / gauge_potential (flows.py:203-211) against
  central differences of the float64 oracle."""
  import oracle
  from cnf_ot_amd import RQSFlow, Params
  for D, scale in ((2, 0.2), (3, 0.15)):
    model = RQSFlow(event_shape=(D,), num_layers=2, hidden_sizes=[16, 16], num_bins=5)
    params = Params.random(model.cfg, scale, seed=40 + D, device=dev)
    ocfg = oracle.OracleConfig(D=D)
    p64 = params.flat.cpu().double().numpy()
    rng = np.random.default_rng(D)
    x = rng.normal(size=(300, D)).astype(np.float32)
    c = np.float32(0.35)
    xt, ct = torch.from_numpy(x).to(dev), torch.tensor([c], device=dev)
    h = 1e-6
    Jf = np.zeros((300, D, D)); Ji = np.zeros((300, D, D)); G = np.zeros((300, D))
    y0, _ = oracle.forward_logdet(ocfg, p64, x.astype(np.float64), [c])
    y32 = y0.astype(np.float32)
    for j in range(D):
      e = np.zeros(D); e[j] = h
      yp, lp = oracle.forward_logdet(ocfg, p64, x + e, [c]); ym, lm = oracle.forward_logdet(ocfg, p64, x - e, [c])
      Jf[:, :, j] = (yp - ym) / (2 * h); G[:, j] = (lp - lm) / (2 * h)
      xp, _ = oracle.inverse_logdet(ocfg, p64, y32 + e, [c]); xm, _ = oracle.inverse_logdet(ocfg, p64, y32 - e, [c])
      Ji[:, :, j] = (xp - xm) / (2 * h)
    jf = model.apply.forward_jac(params, xt, ct).cpu().double().numpy()
    ji = model.apply.inverse_jac(params, torch.from_numpy(y32).to(dev), ct).cpu().double().numpy()
    g = model.apply.gauge_potential(params, xt, ct).cpu().double().numpy()
    g1 = model.apply.gauge_potential(params, xt[0], ct).cpu().double().numpy()
    ef, ei, eg = np.abs(jf - Jf).max(), np.abs(ji - Ji).max(), np.abs(g - G).max()
    print(f"[jac D={D}] forward_jac {ef:.2e} inverse_jac {ei:.2e} gauge_potential {eg:.2e}")
    assert ef <= 2e-5 and ei <= 5e-5 and eg <= 5e-5 and np.abs(g1 - G[0]).max() <= 5e-5
    # the two Jacobians are inverses of each other
    assert np.abs(np.einsum("bij,bjk->bik", jf, ji) - np.eye(D)).max() <= 2e-4


def test_autograd_flow_passes_and_unfused_score_terms(dev):
  """cnf_pass_vjp under torch.autograd: (1) gradient of a host-composed loss ==
  the fused kernel's gradient of the same loss; (2) the unfused dim-10 score
  path == the fused kernel (value and gradient)."""
  from cnf_ot_amd import FlowConfig, FlowModel, Params, _capi
  from cnf_ot_amd import applications as app, autograd as ag
  # (1) dim 2: -mean log_prob of data points, and a sampled potential
  cfg = FlowConfig(dim=2); model = FlowModel(cfg)
  params = Params.random(cfg, 0.2, seed=50, device=dev)
  eng = model.terms_backend(params)
  pts = eng.normal(3, 1000) * 1.3 + 0.2
  flat = params.flat.clone().requires_grad_(True)
  loss = -ag.log_prob(eng, flat, pts, torch.tensor([0.4], device=dev)).double().sum()
  loss.backward()
  g_fused = torch.zeros_like(params.flat)
  s = eng.loss_terms_grad(app._spec(_capi.TERM_NEG_LOGPROB), pts, [0.4], 1000, True, 1.0, g_fused)
  assert abs(float(loss.detach()) - float(s.sum())) <= 1e-6 * abs(float(loss.detach()))
  rel = (flat.grad - g_fused).abs().max().item() / g_fused.abs().max().item()
  print(f"\n[autograd neg_logprob] rel diff vs fused gradient {rel:.2e}")
  assert rel <= 1e-5
  x = eng.normal(4, 1000).requires_grad_(True)
  y, ld = ag.flow_forward(eng, flat, x, torch.tensor([0.7], device=dev))
  (y.pow(2).sum() + ld.sum()).backward()          # exercises the input adjoint too
  assert torch.isfinite(x.grad).all() and x.grad.abs().max() > 0
  # (2) dim 10 score terms: unfused (autograd) vs fused kernel
  cfg10 = FlowConfig(dim=10); m10 = FlowModel(cfg10)
  p10 = Params.random(cfg10, 0.12, seed=51, device=dev)
  B, seed = 2048, 6
  out = {}
  for mode, min_dim in (("unfused", 6), ("fused", 99)):
    app.UNFUSED_SCORE_MIN_DIM = min_dim
    g = torch.zeros_like(p10.flat)
    loss = app.fp_loss_fn(m10, 10, 1.0, 1.0, 0.5, 0.01, 0.01, 2, "ou", p10, seed, 5000.0, B, grad=g)
    loss_ng = app.fp_loss_fn(m10, 10, 1.0, 1.0, 0.5, 0.01, 0.01, 2, "ou", p10, seed, 5000.0, B)
    assert abs(float(loss) - float(loss_ng)) <= 1e-6 * abs(float(loss_ng))
    out[mode] = (float(loss), g.clone())
  app.UNFUSED_SCORE_MIN_DIM = 6
  dl = abs(out["fused"][0] - out["unfused"][0]) / abs(out["fused"][0])
  dg = (out["fused"][1] - out["unfused"][1]).abs().max().item() / out["fused"][1].abs().max().item()
  print(f"[dim10 fp loss] fused {out['fused'][0]:.8g} unfused {out['unfused'][0]:.8g} rel {dl:.2e}; gradient rel {dg:.2e}")
  assert dl <= 1e-5 and dg <= 2e-3


@pytest.mark.parametrize("D,B", [(2, 3000), (3, 1111), (10, 700)])
def test_logprob_fd_score_and_its_backward(dev, D, B):
  """cnf_logprob_fd / cnf_logprob_fd_vjp (the central-difference score of
  applications.py:264-273 with the 2 D evaluation points generated in the
  kernel) against the same thing built from materialised points: the score bit
  for bit (same kernel arithmetic), the backward against torch.autograd over
  cnf_pass_vjp on the materialised points."""
  from cnf_ot_amd import FlowConfig, FlowModel, Params
  from cnf_ot_amd import autograd as ag
  cfg = FlowConfig(dim=D); model = FlowModel(cfg)
  params = Params.random(cfg, 0.2 if D == 2 else 0.12, seed=60 + D, device=dev)
  eng = model.terms_backend(params)
  eng.set_pwl(0)
  dx = 0.01
  r = (eng.normal(7, B) * 1.2).contiguous()
  conds = [torch.tensor([0.35], device=dev), torch.rand(B, device=dev, generator=torch.Generator(device=dev).manual_seed(1))]
  for c in conds:
    per = c.numel() == B
    # materialised evaluation points, ordered (i, d, +/-)
    eye = torch.eye(D, device=dev) * (0.5 * dx)
    pts = torch.stack([r[:, None, :] + eye[None], r[:, None, :] - eye[None]], dim=2).reshape(-1, D).contiguous()
    cc = c.repeat_interleave(2 * D) if per else c
    eng.set_precise(False)
    lp = eng.log_prob(pts, cc).reshape(B, D, 2)
    eng.set_precise(True)
    want = (lp[:, :, 0] - lp[:, :, 1]) * (1.0 / dx)
    got = eng.logprob_fd(r, c, dx)
    assert torch.equal(got, want), (D, per, (got - want).abs().max().item())
    # backward: weights w[i, d] on the score
    w = torch.randn(B, D, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    flat = params.flat.clone().requires_grad_(True)
    rr = r.clone().requires_grad_(True)
    (ag.logprob_fd(eng, flat, rr, c, dx) * w).sum().backward()
    flat2 = params.flat.clone().requires_grad_(True)
    rr2 = r.clone().requires_grad_(True)
    eye2 = eye
    pts2 = torch.stack([rr2[:, None, :] + eye2[None], rr2[:, None, :] - eye2[None]], dim=2).reshape(-1, D)
    eng.set_precise(False)
    lp2 = ag.log_prob(eng, flat2, pts2, cc).reshape(B, D, 2)
    (((lp2[:, :, 0] - lp2[:, :, 1]) * (1.0 / dx)) * w).sum().backward()
    eng.set_precise(True)
    rel_p = (flat.grad - flat2.grad).abs().max().item() / flat2.grad.abs().max().item()
    rel_x = (rr.grad - rr2.grad).abs().max().item() / rr2.grad.abs().max().item()
    print(f"\n[logprob_fd D={D} per_sample_c={per}] param-grad rel {rel_p:.2e}  point-adjoint rel {rel_x:.2e}")
    assert rel_p <= 1e-4 and rel_x <= 1e-4


@pytest.mark.parametrize("D,S,count,drift", [(10, 5, 700, "ou"), (6, 3, 1000, None), (3, 4, 513, "ou"), (2, 2, 2000, None)])
def test_score_fd_vjp_equals_the_three_launch_form(dev, D, S, count, drift):
  """cnf_score_fd_vjp (value AND backward of the score terms of applications.py:245-374 in one launch: the kernel
  that differentiates the 2 D evaluation points forms the score from its own forward passes) against the three
  launches it replaces -- cnf_logprob_fd + cnf_score_residual + cnf_logprob_fd_vjp -- on the same inputs."""
  from cnf_ot_amd import FlowConfig, FlowModel, Params, _capi
  cfg = FlowConfig(dim=D); model = FlowModel(cfg)
  params = Params.random(cfg, 0.2 if D == 2 else 0.12, seed=80 + D, device=dev)
  eng = model.terms_backend(params)
  eng.set_pwl(0)
  n = S * count
  dt, dx, coef, a, loss_coef = 0.01, 0.01, 0.5, 1.3, 0.7 / n
  dr = -1 if drift is None else _capi.DRIFTS[drift]
  t = torch.linspace(0.1, 0.9, S, device=dev)
  z = eng.normal(11, n)
  half = 0.5 * dt
  c3 = torch.cat([t - half, t + half, t])
  r, _ = eng.forward_logdet(z.repeat(3, 1), c3.repeat_interleave(count), want_logdet=False)
  r = r.contiguous()
  # the three-launch form
  g_ref = torch.zeros_like(params.flat)
  r3 = r[2 * n:]
  score = eng.logprob_fd(r3, t, dx)
  sums_ref, rbar_ref, sbar = eng.score_residual(r, score, count, dt, coef, dr, a, loss_coef, True)
  r3bar = eng.logprob_fd_vjp(r3, t, dx, sbar, g_ref)
  rbar_ref[2 * n:] += r3bar
  # one launch
  g = torch.zeros_like(params.flat)
  sums, rbar = eng.score_fd_vjp(r, t, count, dt, dx, coef, dr, a, loss_coef, g)
  torch.cuda.synchronize()
  rel = lambda x, y: (x - y).abs().max().item() / max(y.abs().max().item(), 1e-30)
  e_s, e_r, e_g = rel(sums, sums_ref), rel(rbar, rbar_ref), rel(g, g_ref)
  print(f"\n[score_fd_vjp D={D} drift={drift}] sums rel {e_s:.2e}  rbar rel {e_r:.2e}  grad rel {e_g:.2e}")
  # (the score is a difference of two log_prob values over dx = 0.01: the two forms evaluate the conditioner with
  # different instruction sequences -- packed vector ALU vs matrix cores -- and the difference's rounding is amplified 100 x)
  assert e_s <= 2e-4 and e_r <= 2e-3 and e_g <= 2e-3
  # the same call again: accumulates, bitwise reproducible
  g2 = torch.zeros_like(params.flat)
  sums2, rbar2 = eng.score_fd_vjp(r, t, count, dt, dx, coef, dr, a, loss_coef, g2)
  assert torch.equal(g, g2) and torch.equal(rbar, rbar2)


@pytest.mark.parametrize("L,S,Bs", [(2, 5, 6002), (3, 70, 1500)])
@pytest.mark.parametrize("to_base", [False, True])
def test_pass_vjp_table_form_matches_mlp_backward(dev, to_base, L, S, Bs):
  """cnf_pass_vjp at dim 2 on the conditioner tables: per-piece sufficient statistics (A = sum theta_bar,
  B = sum (u - u_ref) theta_bar) instead of per-sample weight gradients (algebra restated and checked
  on the CPU in oracle/pwl_grad.py).  Same input adjoints and the same parameter gradient as the MLP backward, on
  slices of ragged length with a partial last slice."""
  from cnf_ot_amd import FlowConfig, FlowEngine, Params
  cfg = FlowConfig(dim=2, num_layers=L)      # (L = 3, 70 slices: two chunks of the 64-slice statistics buffer)
  params = Params.random(cfg, 0.2, seed=5, device=dev)
  eng = FlowEngine(cfg, dev).load(params)
  gen = torch.Generator(device="cpu").manual_seed(3)
  B = S * Bs                                 # slices of full tiles of 1 024 + a partial one
  pts = torch.randn(B, 2, generator=gen).to(dev) * (1.0 if not to_base else 1.5)
  ts = torch.linspace(0.1, 0.9, S).to(dev)
  ybar = torch.randn(B, 2, generator=gen).to(dev)
  ldbar = torch.randn(B, generator=gen).to(dev)
  c_host = ts.repeat_interleave(Bs)[:B].contiguous()
  res = {}
  for mode in (0, 2):
    eng.set_pwl(mode)
    g = torch.zeros(cfg.param_count(), device=dev)
    # mode 0: per-sample conditions (the MLP backward); mode 2: the slices' conditions, c_block = Bs
    xbar = eng.pass_vjp(pts, ts if mode == 2 else c_host[:, None], ybar, ldbar, to_base, grad=g)
    torch.cuda.synchronize()
    res[mode] = (xbar, g, eng.last_path())
  assert res[2][2] == "tables" and res[0][2] != "tables"
  # fixed-point statistics and one owner per slab: the same bits every time
  eng.set_pwl(2)
  g_again = torch.zeros(cfg.param_count(), device=dev)
  eng.pass_vjp(pts, ts, ybar, ldbar, to_base, grad=g_again, want_xbar=False)
  assert torch.equal(g_again, res[2][1])
  xb0, g0, _ = res[0]; xb2, g2, _ = res[2]
  ex = (xb2 - xb0).abs().max().item() / xb0.abs().max().item()
  eg = (g2 - g0).abs().max().item() / g0.abs().max().item()
  print(f"\n[pass_vjp tables vs mlp, to_base={to_base}] xbar rel {ex:.2e}  grad rel {eg:.2e}  |g|inf {g0.abs().max().item():.3g}")
  assert ex <= 2e-5 and eg <= 5e-5
  # the `first` block and every tensor of a conditioner individually (a wrong row would hide in the maximum)
  blocks = [(0, 16)]
  for l in range(L):
    o = 16 + 592 * l
    blocks += [(o, o + 32), (o + 32, o + 48), (o + 48, o + 304), (o + 304, o + 320), (o + 320, o + 576), (o + 576, o + 592)]
  for lo, hi in blocks:
    ref = g0[lo:hi].abs().max().item()
    assert (g2[lo:hi] - g0[lo:hi]).abs().max().item() <= 1e-4 * max(ref, 1e-3 * g0.abs().max().item()), (lo, hi)


# (slice length, slices, passes) -> composed from table launches in the default mode?  From the predicate the loss code
# used to evaluate itself: count >= 8 192 and count * slices * passes >= 262 144.
TABLE_ROUTES = [(65536, 1, 1, False), (262144, 1, 1, True), (131072, 1, 1, False), (131072, 1, 2, True),
                (8192, 32, 1, True), (8192, 16, 2, True), (8191, 64, 1, False), (4096, 96, 2, False)]


def test_table_route_query_in_the_default_mode(dev):
  """cnf_model_term_on_tables (FlowEngine.term_on_tables) in the default table mode: the routes the loss code took
  when it kept its own copy of the thresholds, for the value alone and with the gradient; never at dim 3, with
  set_pwl(0), or -- with the gradient -- for 5 flow layers (the table backward exists for up to 4).  cnf_pass_vjp takes
  the route the query names."""
  from cnf_ot_amd import FlowConfig, FlowEngine, Params

  def engine(**kw):
    cfg = FlowConfig(**kw)
    params = Params.random(cfg, 0.2, seed=6, device=dev)
    eng = FlowEngine(cfg, dev).load(params)
    eng.grad_ready(torch.zeros_like(params.flat))
    return cfg, eng

  cfg, eng = engine(dim=2)
  _, eng3 = engine(dim=3)
  _, eng5 = engine(dim=2, num_layers=5)
  for count, S, passes, want in TABLE_ROUTES:
    n = count * S * passes
    assert want == (count >= 8192 and n >= 262144)
    for with_grad in (False, True):
      assert eng.term_on_tables(count, n, with_grad) == want, (count, S, passes, with_grad)
      assert not eng3.term_on_tables(count, n, with_grad)
      eng.set_pwl(0)
      assert not eng.term_on_tables(count, n, with_grad)
      eng.set_pwl(1)
    assert not eng5.term_on_tables(count, n, True)
  gen = torch.Generator(device="cpu").manual_seed(3)
  for B in (65536, 262144):      # a "no" shape first: the MLP backward leaves last_path alone
    pts = torch.randn(B, 2, generator=gen).to(dev)
    ybar = torch.randn(B, 2, generator=gen).to(dev)
    g = torch.zeros(cfg.param_count(), device=dev)
    eng.pass_vjp(pts, torch.tensor([0.4], device=dev), ybar, None, False, grad=g, want_xbar=False)
    torch.cuda.synchronize()
    assert (eng.last_path() == "tables") == eng.term_on_tables(B, B, True), B
    assert torch.isfinite(g).all() and g.abs().max().item() > 0


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_table_backward_does_not_hide_non_finite_adjoints(dev, bad):
  """The fixed-point statistics of the table backward cannot carry a NaN or an Inf (an integer sum, range tests that
  drop what they cannot represent): a call that meets one flags it and answers with a NaN gradient -- what the float
  accumulation of the MLP backward gives, and what a training loop looks for.  The next call is clean again."""
  from cnf_ot_amd import FlowConfig, FlowEngine, Params
  cfg = FlowConfig(dim=2)
  params = Params.random(cfg, 0.2, seed=5, device=dev)
  eng = FlowEngine(cfg, dev).load(params)
  S, Bs = 4, 3000
  gen = torch.Generator(device="cpu").manual_seed(3)
  pts = torch.randn(S * Bs, 2, generator=gen).to(dev)
  ts = torch.linspace(0.1, 0.9, S).to(dev)
  ybar = torch.randn(S * Bs, 2, generator=gen).to(dev)
  good = ybar.clone()
  ybar[1234, 1] = bad
  eng.set_pwl(2)
  g = torch.zeros(cfg.param_count(), device=dev)
  eng.pass_vjp(pts, ts, ybar, None, False, grad=g, want_xbar=False)
  assert eng.last_path() == "tables"
  assert not torch.isfinite(g).all()
  eng.set_pwl(0)
  g_mlp = torch.zeros(cfg.param_count(), device=dev)
  eng.pass_vjp(pts, ts.repeat_interleave(Bs)[:, None], ybar, None, False, grad=g_mlp, want_xbar=False)
  assert not torch.isfinite(g_mlp).all()
  eng.set_pwl(2)
  g2 = torch.zeros(cfg.param_count(), device=dev)
  eng.pass_vjp(pts, ts, good, None, False, grad=g2, want_xbar=False)
  assert torch.isfinite(g2).all() and g2.abs().max().item() > 0
  eng.set_pwl(1)


@pytest.mark.parametrize("subtype", ["free", "obstacle", "rwpo"])
def test_value_and_grad_through_the_table_backward(dev, subtype, monkeypatch):
  """ot_loss_fn at dim 2 with its terms composed from table-path launches + cnf_pass_vjp on the tables
  (applications._neg_logprob_tables / _kinetic_tables / _potential_tables; chosen for large batches, forced here):
  same loss and the same gradient as the fused gradient kernel."""
  from cnf_ot_amd import RQSFlow, Params, applications as app
  model = RQSFlow(event_shape=(2,), num_layers=2, hidden_sizes=[16, 16], num_bins=5)
  params = Params.random(model.cfg, 0.15, seed=9, device=dev)
  B, tbs = 65536, 3
  if subtype == "rwpo":      # reverse KL + potential through the tables (the finite-difference score term stays fused)
    f = lambda p, rng, lam, bs, **kw: app.rwpo_loss_fn(model, 2, 1.0, 1.0, 0.01, 0.01, tbs, "quadratic", 1.0, p, rng, lam, bs, **kw)
  else:
    f = lambda p, rng, lam, bs, **kw: app.ot_loss_fn(model, 2, 1.0, 0.01, tbs, subtype, p, rng, lam, bs, source="gaussian", **kw)
  vg = app.value_and_grad(f)
  be = model.terms_backend(params)
  be.set_pwl(0)
  loss0, g0 = vg(params, 11, 50.0, B)
  used = []
  orig, orig_nlp, orig_kp = be.pass_vjp, be.neg_logprob_vjp, be.kinetic_potential_vjp
  monkeypatch.setattr(be, "pass_vjp", lambda *a, **k: (used.append(1), orig(*a, **k))[1])
  monkeypatch.setattr(be, "neg_logprob_vjp", lambda *a, **k: (used.append(1), orig_nlp(*a, **k))[1])
  monkeypatch.setattr(be, "kinetic_potential_vjp", lambda *a, **k: (used.append(1), orig_kp(*a, **k))[1])
  be.set_pwl(2)
  loss2, g2 = vg(params, 11, 50.0, B)
  torch.cuda.synchronize()
  be.set_pwl(1)
  assert len(used) >= (2 if subtype == "rwpo" else 3)      # two density-fit terms + kinetic (+ obstacle); rkl + potential
  el = abs(float(loss2) - float(loss0)) / abs(float(loss0))
  eg = (g2.flat - g0.flat).abs().max().item() / g0.flat.abs().max().item()
  print(f"\n[ot {subtype}: table backward vs fused kernel] loss rel {el:.2e} grad rel {eg:.2e}")
  assert el <= 2e-5 and eg <= 2e-4


@pytest.mark.parametrize("subtype", ["free", "obstacle"])
def test_loss_without_gradient_through_the_tables(dev, subtype, monkeypatch):
  """ot_loss_fn WITHOUT a gradient at a large dim-2 batch (forced here): its terms composed from the table forward and
  the term epilogues (cnf_kinetic_potential_vjp with grad = NULL; cnf_inverse_logdet + cnf_term_residual) -- the same
  loss as the fused loss kernel, and as the value the gradient path returns."""
  from cnf_ot_amd import RQSFlow, Params, applications as app
  model = RQSFlow(event_shape=(2,), num_layers=2, hidden_sizes=[16, 16], num_bins=5)
  params = Params.random(model.cfg, 0.15, seed=9, device=dev)
  B, tbs = 65536, 3
  f = lambda p, rng, lam, bs, **kw: app.ot_loss_fn(model, 2, 1.0, 0.01, tbs, subtype, p, rng, lam, bs, source="gaussian", **kw)
  be = model.terms_backend(params)
  be.set_pwl(0)
  loss0 = float(f(params, 11, 50.0, B))
  used = []
  orig_kp = be.kinetic_potential_vjp
  monkeypatch.setattr(be, "kinetic_potential_vjp", lambda *a, **k: (used.append(a[5] is None), orig_kp(*a, **k))[1])
  be.set_pwl(2)
  loss2 = float(f(params, 11, 50.0, B))
  lossg, _ = app.value_and_grad(f)(params, 11, 50.0, B)
  torch.cuda.synchronize()
  be.set_pwl(1)
  assert used == [True, False]      # values alone, then with the gradient
  e0, eg = abs(loss2 - loss0) / abs(loss0), abs(loss2 - float(lossg)) / abs(loss0)
  print(f"\n[ot {subtype}: loss on the tables vs fused kernel] rel {e0:.2e}; vs the gradient path's value {eg:.2e}")
  assert e0 <= 2e-5 and eg <= 1e-6


def test_fused_term_calls_decline_flag_and_recover(dev):
  """cnf_neg_logprob_vjp / cnf_kinetic_potential_vjp at their edges: below the table backward's thresholds (default
  table mode) and past 128 slices they decline (None: the caller composes the term) and leave the gradient untouched;
  a non-finite data point or draw turns the call's gradient into NaN (as the composed path does:
  test_table_backward_does_not_hide_non_finite_adjoints) and the next call is clean; odd slice lengths decline."""
  from cnf_ot_amd import FlowConfig, FlowEngine, Params
  cfg = FlowConfig(dim=2)
  params = Params.random(cfg, 0.2, seed=6, device=dev)
  eng = FlowEngine(cfg, dev).load(params)
  gen = torch.Generator(device="cpu").manual_seed(8)
  n = 20000
  pts = torch.randn(n, 2, generator=gen).to(dev)
  z = torch.randn(n, 2, generator=gen).to(dev)
  g = torch.zeros(cfg.param_count(), device=dev)
  t1 = torch.tensor([0.3], device=dev)
  c2 = torch.tensor([0.295, 0.305], device=dev)
  # default table mode: 20 000 points are below the thresholds
  assert eng.neg_logprob_vjp(pts, t1, 0.01, g) is None
  assert eng.kinetic_potential_vjp(z, c2, 1, 0.01, 0.5, g) is None
  assert g.abs().max().item() == 0.0
  eng.set_pwl(2)
  # more slices than one chunk of statistics (kinetic: 2 S > 128), an odd slice length with several slices
  zs = z[:1024].contiguous()
  assert eng.kinetic_potential_vjp(zs, torch.linspace(0.1, 0.9, 130, device=dev), 65, 0.01, 0.5, g) is None
  assert eng.kinetic_potential_vjp(z[:9001].contiguous(), c2, 1, 0.01, 0.5, g) is None
  assert g.abs().max().item() == 0.0
  # a non-finite input: NaN gradient, then a clean call
  for bad in (float("nan"), float("inf")):
    p2 = pts.clone(); p2[777, 0] = bad
    gb = torch.zeros_like(g)
    assert eng.neg_logprob_vjp(p2, t1, 0.01, gb) is not None
    assert not torch.isfinite(gb).all()
    z2 = z.clone(); z2[4321, 1] = bad
    gb = torch.zeros_like(g)
    assert eng.kinetic_potential_vjp(z2, c2, 1, 0.01, 0.5, gb) is not None
    assert not torch.isfinite(gb).all()
    for call in (lambda gg: eng.neg_logprob_vjp(pts, t1, 0.01, gg), lambda gg: eng.kinetic_potential_vjp(z, c2, 1, 0.01, 0.5, gg)):
      gc = torch.zeros_like(g)
      assert call(gc) is not None
      assert torch.isfinite(gc).all() and gc.abs().max().item() > 0
  eng.set_pwl(1)


@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("subtype", [None, "obstacle", "double_well"])
@pytest.mark.parametrize("S,count", [(1, 70002), (5, 9000), (32, 8194)])
def test_kinetic_potential_vjp_equals_the_composed_terms(dev, subtype, S, count, L):
  """cnf_kinetic_potential_vjp (kinetic_loss_fn + potential_loss_fn as ot_loss_fn combines them, applications.py:176-242,
  388-402, under jax.value_and_grad) against the same terms composed from cnf_sample on repeated copies of z +
  cnf_term_residual + cnf_pass_vjp: the same tables, kernels and adjoints, so sums to 1e-12 and the gradient BIT FOR BIT."""
  from cnf_ot_amd import FlowConfig, FlowEngine, Params, _capi
  cfg = FlowConfig(dim=2, num_layers=L)
  params = Params.random(cfg, 0.2, seed=4, device=dev)
  eng = FlowEngine(cfg, dev).load(params)
  eng.set_pwl(2)
  g = torch.Generator(device="cpu").manual_seed(S + count)
  z = torch.randn(count, 2, generator=g).to(dev)
  t = torch.linspace(0.1, 0.9, S, device=dev)
  dt, c_kin, c_pot, a = 0.01, 0.37 / count, 0.11 / count, 1.5
  half = np.float32(0.5 * dt)
  sets = [t - half, t + half] + ([t] if subtype else [])
  c = torch.cat(sets).contiguous()
  n = S * count
  g1 = torch.zeros(cfg.param_count(), device=dev)
  out = eng.kinetic_potential_vjp(z, c, S, dt, c_kin, g1, subtype=_capi.POTENTIALS[subtype] if subtype else -1, a=a, c_pot=c_pot)
  assert out is not None and eng.last_path() == "tables"
  kin1, pot1 = out
  zr = z.repeat(len(sets) * S, 1)
  r, _ = eng.forward_logdet(zr, c, want_logdet=False)
  rbar = torch.empty_like(r)
  kin0, _, _ = eng.term_residual(_capi.TERM_KINETIC, r[:2 * n], None, count, p0=dt, loss_coef=c_kin, rbar_out=rbar[:2 * n])
  if subtype:
    pot0, _, _ = eng.term_residual(_capi.TERM_POTENTIAL, r[2 * n:], None, count, subtype=_capi.POTENTIALS[subtype], p0=a,
                                   loss_coef=c_pot, rbar_out=rbar[2 * n:])
  g0 = torch.zeros_like(g1)
  eng.pass_vjp(zr, c, rbar, None, False, grad=g0, want_xbar=False)
  torch.cuda.synchronize()
  torch.testing.assert_close(kin1, kin0, rtol=1e-12, atol=0)
  if subtype:
    torch.testing.assert_close(pot1, pot0, rtol=1e-12, atol=0)
  else:
    assert pot1 is None
  assert torch.equal(g1, g0)
  # grad = None: the values alone, the same sums
  out = eng.kinetic_potential_vjp(z, c, S, dt, c_kin, None, subtype=_capi.POTENTIALS[subtype] if subtype else -1, a=a, c_pot=c_pot)
  torch.cuda.synchronize()
  torch.testing.assert_close(out[0], kin0, rtol=1e-12, atol=0)
  if subtype:
    torch.testing.assert_close(out[1], pot0, rtol=1e-12, atol=0)


@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("S,Bs", [(1, 70001), (3, 9000), (5, 8194), (130, 1024)])
def test_neg_logprob_vjp_equals_the_composed_term(dev, L, S, Bs):
  """cnf_neg_logprob_vjp (kl_loss_fn under jax.value_and_grad, applications.py:11-86 / solvers.py:94: the table
  backward seeding itself with ybar = coef x, ldbar = -coef) against the same term composed from cnf_inverse_logdet +
  cnf_term_residual + cnf_pass_vjp: per-slice sums to 2e-6, gradient to 1e-5 of its largest entry.  Slices that end inside
  a tile and inside a lane's sample pair, more slices than one chunk of statistics, a third flow layer."""
  from cnf_ot_amd import FlowConfig, FlowEngine, Params, _capi
  cfg = FlowConfig(dim=2, num_layers=L)
  params = Params.random(cfg, 0.2, seed=3, device=dev)
  eng = FlowEngine(cfg, dev).load(params)
  eng.set_pwl(2)
  B = S * Bs
  g = torch.Generator(device="cpu").manual_seed(S * 7 + Bs)
  pts = (torch.randn(B, 2, generator=g) * 1.3).to(dev)
  ts = torch.linspace(0.05, 0.95, S, device=dev)
  coef = 0.013
  g1 = torch.zeros(cfg.param_count(), device=dev)
  sums1 = eng.neg_logprob_vjp(pts, ts, coef, g1)
  assert sums1 is not None and eng.last_path() == "tables"
  eng.set_precise(False)
  x, ildj = eng.inverse_logdet(pts, ts)
  eng.set_precise(True)
  sums0, xbar, ldbar = eng.term_residual(_capi.TERM_NEG_LOGPROB, x, ildj, Bs, loss_coef=coef)
  g0 = torch.zeros_like(g1)
  eng.pass_vjp(pts, ts, xbar, ldbar, True, grad=g0, want_xbar=False)
  torch.cuda.synchronize()
  es = ((sums1 - sums0).abs() / sums0.abs()).max().item()
  eg = (g1 - g0).abs().max().item() / g0.abs().max().item()
  print(f"\n[neg_logprob_vjp L={L} {S} x {Bs}] sums rel {es:.2e} grad rel {eg:.2e}")
  assert es <= 2e-6 and eg <= 1e-5
  # accumulates into grad, and is bitwise reproducible
  g2 = torch.zeros_like(g1)
  sums2 = eng.neg_logprob_vjp(pts, ts, coef, g2)
  torch.cuda.synchronize()
  assert torch.equal(g2, g1)
  torch.testing.assert_close(sums2, sums1, rtol=1e-12, atol=0)


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("n,count", [(10000, 10000), (9999, 1234), (70001, 4096), (5000, 1), (300000, 131072)])
def test_term_residual_sums_and_adjoints(dev, D, n, count):
  """cnf_term_residual (the epilogue of the table-backward terms: applications.py:176-205, 220-242, 85) against a
  float64 torch restatement: per-slice sums to 2e-6 relative, adjoints to float32 rounding.  Slices that end inside
  a wave, inside a workgroup's four-point stride and past the last workgroup are all in the cases."""
  from cnf_ot_amd import FlowConfig, FlowEngine, Params, _capi
  cfg = FlowConfig(dim=D)
  eng = FlowEngine(cfg, dev).load(Params.random(cfg, 0.1, seed=1, device=dev))
  g = torch.Generator(device="cpu").manual_seed(n + D)
  n_slices = -(-n // count)
  coef = 0.37

  def slice_sums(v):
    pad = torch.zeros(n_slices * count, dtype=torch.float64)
    pad[:n] = v
    return pad.view(n_slices, count).sum(1)

  def check(sums, want):
    # (the values are float32 per point: a one-point slice carries that rounding, relative to the term's scale)
    torch.testing.assert_close(sums.cpu(), want, rtol=2e-6, atol=2e-6 * float(want.abs().max()) / min(count, 100))

  # kinetic: r = [r1; r2], v = (r2 - r1) / dt
  r = (torch.randn(2 * n, D, generator=g) * 1.5).to(dev)
  dt = 0.01
  sums, rbar, _ = eng.term_residual(_capi.TERM_KINETIC, r, None, count, p0=dt, loss_coef=coef)
  r64 = r.cpu().double()
  dr = r64[n:] - r64[:n]
  check(sums, slice_sums(((dr / dt) ** 2).sum(1)))
  gref = 2 * coef * dr / dt ** 2
  torch.testing.assert_close(rbar.cpu().double(), torch.cat([-gref, gref]), rtol=2e-6, atol=1e-6)
  # potentials
  x = (torch.randn(n, D, generator=g) * 1.2).to(dev)
  x64 = x.cpu().double()
  for name, sub in _capi.POTENTIALS.items():
    p0 = 1.5 if name == "double_well" else 0.0
    sums, xbar, _ = eng.term_residual(_capi.TERM_POTENTIAL, x, None, count, subtype=sub, p0=p0, loss_coef=coef)
    xr = x64.clone().requires_grad_(True)
    if name == "double_well": v = 0.25 * ((xr - p0) ** 2).sum(1) * ((xr + p0) ** 2).sum(1)
    elif name == "obstacle": v = 50.0 * torch.exp(-0.5 * (xr ** 2).sum(1))
    else: v = 0.5 * (xr ** 2).sum(1)
    check(sums, slice_sums(v.detach()))
    (coef * v.sum()).backward()
    torch.testing.assert_close(xbar.cpu().double(), xr.grad, rtol=5e-6, atol=1e-5)
  # density fit: -(ld + base log-density of y)
  ld = torch.randn(n, generator=g).to(dev)
  sums, ybar, ldbar = eng.term_residual(_capi.TERM_NEG_LOGPROB, x, ld, count, loss_coef=coef)
  v = -(ld.cpu().double() - 0.5 * (x64 ** 2).sum(1) - 0.5 * D * np.log(2 * np.pi))
  check(sums, slice_sums(v))
  torch.testing.assert_close(ybar.cpu().double(), coef * x64, rtol=1e-6, atol=1e-7)
  assert torch.all(ldbar == -coef)


@pytest.mark.parametrize("to_base", [False, True])
def test_table_backward_properties_at_config5_size(dev, to_base):
  """The table backward at config 5's per-GPU share (32 slices x 131 072 points), through properties that need no
  oracle at that size: (a) the same bits on a second call; (b) adjoints scaled by a power of two scale the
  fixed-point statistics' scale with them, so gradient and input adjoints scale EXACTLY; (c) the gradient is a sum
  over slices: the two halves of the time batch add up to the whole (float sums in another order: 2e-6)."""
  from cnf_ot_amd import FlowConfig, FlowEngine, Params
  cfg = FlowConfig(dim=2)
  eng = FlowEngine(cfg, dev).load(Params.random(cfg, 0.2, seed=11, device=dev))
  eng.set_pwl(2)
  S, Bs = 32, 131072
  B = S * Bs
  gen = torch.Generator(device=dev).manual_seed(7)
  pts = torch.randn(B, 2, generator=gen, device=dev) * 1.3
  ybar = torch.randn(B, 2, generator=gen, device=dev)
  ldbar = torch.randn(B, generator=gen, device=dev)
  ts = torch.linspace(0.02, 0.98, S, device=dev)

  def run(lo, hi, scale=1.0):
    g = torch.zeros(cfg.param_count(), device=dev)
    sl = slice(lo * Bs, hi * Bs)
    xb = eng.pass_vjp(pts[sl], ts[lo:hi].contiguous(), ybar[sl] * scale, ldbar[sl] * scale, to_base, grad=g)
    assert eng.last_path() == "tables"
    return xb, g

  xb, g = run(0, S)
  xb2, g2 = run(0, S)
  assert torch.equal(g, g2) and torch.equal(xb, xb2)
  xb4, g4 = run(0, S, 4.0)
  assert torch.equal(g4, g * 4.0) and torch.equal(xb4, xb * 4.0)
  _, ga = run(0, S // 2)
  _, gb = run(S // 2, S)
  assert ((ga + gb) - g).abs().max().item() <= 2e-6 * g.abs().max().item()
  assert torch.isfinite(g).all() and g.abs().max().item() > 0


def test_inverse_direction_backward_next_to_a_knot(dev):
  """Regression (found by scripts/soak_vjp_tables.py, seed 1 case 16): base -> data samples whose conditioned spline
  lands within a rounding of a knot.  The backward used the forward pass's output with its own, differently rounded
  knots; the position clipped and the implicit-function quotient gave input adjoints of 3e9 where the float64
  oracle's central differences give 0.02.  Both backward kernels (MLP and tables) against those differences."""
  import oracle
  from cnf_ot_amd import FlowConfig, FlowEngine, Params
  cfg = FlowConfig(dim=2); ocfg = oracle.OracleConfig(D=2)
  rng = np.random.default_rng(1)
  for case in range(17):                       # the soak's draws, up to its case 16
    scale = float(rng.choice([0.05, 0.1, 0.2, 0.3, 0.5, 0.8, 1.5]))
    spread = float(rng.choice([1.0, 2.0, 4.0, 6.0]))
    amag = float(10.0 ** rng.uniform(-6, 4))
    w = rng.normal(0, scale, cfg.param_count()).astype(np.float32)
    S, Bs = 4, 9000
    B = S * Bs
    pts = rng.normal(0, spread, (B, 2)).astype(np.float32)
    ybar = (rng.normal(0, 1, (B, 2)) * amag).astype(np.float32)
    ldbar = (rng.normal(0, 1, B) * amag).astype(np.float32)
    ts = rng.uniform(0, 1, S).astype(np.float32)
  assert (scale, spread) == (0.5, 6.0)
  eng = FlowEngine(cfg, dev).load(Params(cfg, torch.from_numpy(w).to(dev)))
  t_dev = torch.from_numpy(ts).to(dev)
  c_host = np.repeat(ts.astype(np.float64), Bs)
  h = 1e-6
  for mode in (0, 2):
    eng.set_pwl(mode)
    g = torch.zeros(cfg.param_count(), device=dev)
    xb = eng.pass_vjp(torch.from_numpy(pts).to(dev), t_dev if mode == 2 else t_dev.repeat_interleave(Bs)[:, None],
                      torch.from_numpy(ybar).to(dev), torch.from_numpy(ldbar).to(dev), False, grad=g)
    xb = xb.cpu().double().numpy()
    assert np.isfinite(xb).all() and np.abs(xb).max() < 1e3, np.abs(xb).max()       # was 3.2e9
    for i in (1096, 7700, 8733):
      ref = np.zeros(2)
      for e in range(2):
        xp = pts[i:i + 1].astype(np.float64).copy(); xm = xp.copy(); xp[0, e] += h; xm[0, e] -= h
        yp, lp = oracle.forward_logdet(ocfg, w.astype(np.float64), xp, c_host[i:i + 1])
        ym, lm = oracle.forward_logdet(ocfg, w.astype(np.float64), xm, c_host[i:i + 1])
        ref[e] = ((yp - ym)[0] @ ybar[i].astype(np.float64) + (lp - lm)[0] * float(ldbar[i])) / (2 * h)
      # an ill-conditioned flow (parameter scale 0.5, points out to |x| = 16) in float32: the right magnitude and sign
      assert np.abs(xb[i] - ref).max() <= 0.6 * np.abs(ref).max() + 1e-4, (mode, i, xb[i], ref)


@pytest.mark.parametrize("to_base", [False, True])
def test_input_adjoints_on_the_linear_tails(dev, to_base):
  """Regression (scripts/soak_xbar_oracle.py): on the UPPER linear tail the spline hangs on the fixed corner (hi, hi),
  not on the last knot's y -- the backward fed the output adjoint into the heights' softmax there, and the adjoint
  of the conditioner's input was off by O(1) for every sample beyond +10.  Points spread to |x| ~ 20, both kernels,
  against central differences of the float64 oracle (samples on a kink of the float64 function excluded)."""
  import oracle
  from cnf_ot_amd import FlowConfig, FlowEngine, Params
  cfg = FlowConfig(dim=2); ocfg = oracle.OracleConfig(D=2)
  rng = np.random.default_rng(5)
  S, Bs = 4, 9000
  B = S * Bs
  w = rng.normal(0, 0.25, cfg.param_count()).astype(np.float32)
  pts = rng.normal(0, 6.0, (B, 2)).astype(np.float32)
  ybar = rng.normal(0, 1, (B, 2)).astype(np.float32)
  ldbar = rng.normal(0, 1, B).astype(np.float32)
  ts = rng.uniform(0, 1, S).astype(np.float32)
  c_host = np.repeat(ts.astype(np.float64), Bs)
  fn = oracle.inverse_logdet if to_base else oracle.forward_logdet
  w64 = w.astype(np.float64)

  def fd(h):
    ref = np.zeros((B, 2))
    for e in range(2):
      xp = pts.astype(np.float64).copy(); xm = xp.copy(); xp[:, e] += h; xm[:, e] -= h
      yp, lp = fn(ocfg, w64, xp, c_host); ym, lm = fn(ocfg, w64, xm, c_host)
      ref[:, e] = (((yp - ym) * ybar).sum(1) + (lp - lm) * ldbar) / (2 * h)
    return ref

  r1, r2 = fd(1e-6), fd(3e-6)
  mag = np.abs(r1).max(1) + 1e-3 * np.median(np.abs(r1).max(1))
  smooth = np.abs(r1 - r2).max(1) <= 1e-3 * mag
  tail = (np.abs(pts) > 10).any(1)
  assert tail.sum() > 3000 and smooth.sum() > 0.99 * B
  # base -> data: an output within 1e-3 of the range's edge is a position float32 resolves to 1e-3 of its distance from
  # the knot, and the log-det partials there carry that (3 .. 20 % on ~150 samples of this set: scripts/debug_xbar_tail.py);
  # the float64 reference has no such limit -- those samples are left to the soak's report
  y64, _ = fn(ocfg, w64, pts.astype(np.float64), c_host)
  resolved = (np.abs(np.abs(y64) - 10.0) > 1e-3).all(1)
  smooth &= resolved
  eng = FlowEngine(cfg, dev).load(Params(cfg, torch.from_numpy(w).to(dev)))
  t_dev = torch.from_numpy(ts).to(dev)
  for mode in (0, 2):
    eng.set_pwl(mode)
    g = torch.zeros(cfg.param_count(), device=dev)
    xb = eng.pass_vjp(torch.from_numpy(pts).to(dev), t_dev if mode == 2 else t_dev.repeat_interleave(Bs)[:, None],
                      torch.from_numpy(ybar).to(dev), torch.from_numpy(ldbar).to(dev), to_base, grad=g).cpu().double().numpy()
    rel = np.where(smooth, np.abs(xb - r1).max(1) / mag, 0.0)
    print(f"\n[tails to_base={to_base} mode={mode}] tail samples {int(tail.sum())}: worst rel {rel[tail].max():.2e}; "
          f"all: median {np.median(rel):.1e}, beyond 1% {int((rel > 1e-2).sum())}")
    assert rel[tail].max() <= 2e-2 and (rel > 1e-2).sum() <= 5


def test_term_specs_outside_the_reference_are_rejected(dev):
  """The C ABI checks a term spec the same way in every entry point that takes one (cnf_loss_terms and
  cnf_loss_terms_grad alike): a potential subtype outside 0..2, a drift subtype outside 0..3 (-1..3 where -1 means no
  drift), a reverse-KL term with T <= 0 or beta <= 0 return CNF_ERR_INVALID, on real device buffers."""
  from cnf_ot_amd import FlowConfig, FlowEngine, Params, _capi
  from cnf_ot_amd.flows import _stream_ptr
  cfg = FlowConfig(dim=2)
  params = Params.random(cfg, 0.2, seed=5, device=dev)
  eng = FlowEngine(cfg, dev).load(params)
  lib, h, st = eng.lib, eng._h, _stream_ptr(dev)
  assert lib.cnf_grad_enable(h, 0) == _capi.CNF_OK
  B, inv = 64, _capi.CNF_ERR_INVALID
  pts = torch.randn(B, 2, device=dev)
  t = torch.full((1,), 0.5, device=dev)
  sums = torch.zeros(4, dtype=torch.float64, device=dev)
  grad = torch.zeros(cfg.param_count(), device=dev)
  flat = params.flat.contiguous()
  S = _capi.CnfLossSpec
  bad = [S(kind=_capi.TERM_POTENTIAL, subtype=3, a=1.0),
         S(kind=_capi.TERM_FLOW_MATCHING, subtype=4, dt=0.01, dx=0.01, coef=1.0, a=1.0),
         S(kind=_capi.TERM_REVERSE_KL, T=0.0, beta=1.0),
         S(kind=_capi.TERM_REVERSE_KL, T=1.0, beta=0.0)]
  for spec in bad:
    assert lib.cnf_loss_terms(h, _capi.ctypes.byref(spec), pts.data_ptr(), 0, t.data_ptr(), 1, B, sums.data_ptr(),
                              st) == inv, (spec.kind, spec.subtype)
    assert lib.cnf_loss_terms_grad(h, _capi.ctypes.byref(spec), pts.data_ptr(), 0, t.data_ptr(), 1, B, 1.0,
                                   sums.data_ptr(), grad.data_ptr(), flat.data_ptr(), st) == inv, (spec.kind, spec.subtype)
  # several terms: every spec is checked before the first term's sums are touched
  ct = _capi.ctypes
  two = (S * 2)(S(kind=_capi.TERM_KINETIC, dt=0.01), bad[0])
  sums2 = torch.full((2,), 7.0, dtype=torch.float64, device=dev)
  P2 = ct.c_void_p * 2
  assert lib.cnf_loss_terms_grad_multi(h, 2, two, P2(pts.data_ptr(), pts.data_ptr()), (ct.c_int32 * 2)(0, 0),
                                       P2(t.data_ptr(), t.data_ptr()), (ct.c_int64 * 2)(1, 1), (ct.c_int64 * 2)(B, B),
                                       (ct.c_float * 2)(1.0, 1.0), P2(sums2.data_ptr(), sums2[1:].data_ptr()),
                                       grad.data_ptr(), flat.data_ptr(), st) == inv
  out = torch.zeros(B, 2, device=dev)
  assert lib.cnf_term_residual(_capi.TERM_POTENTIAL, pts.data_ptr(), None, B, B, 2, 3, 1.0, 1.0, sums.data_ptr(),
                               out.data_ptr(), None, st) == inv
  c = torch.tensor([0.45, 0.55, 0.5], device=dev)
  work = torch.zeros(16 * B, device=dev)
  assert lib.cnf_kinetic_potential_vjp(h, pts.data_ptr(), B, c.data_ptr(), 1, 0.1, 1.0, 3, 1.0, 1.0, sums.data_ptr(),
                                       sums[1:].data_ptr(), None, None, work.data_ptr(), st) == inv
  r = torch.randn(3 * B, 2, device=dev)
  score, rbar, sbar = torch.zeros(B, 2, device=dev), torch.zeros(3 * B, 2, device=dev), torch.zeros(B, 2, device=dev)
  assert lib.cnf_score_residual(r.data_ptr(), score.data_ptr(), B, B, 2, 0.01, 1.0, -2, 1.0, 1.0, sums.data_ptr(),
                                rbar.data_ptr(), sbar.data_ptr(), st) == inv
  torch.cuda.synchronize()
  assert not sums.any() and not grad.any() and not out.any() and not work.any() and not rbar.any()
  assert (sums2 == 7.0).all()
