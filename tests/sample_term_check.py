"""What the three test_training_term_against_the_float64_adjoint tests (test_gpu_mmd.py, test_gpu_sinkhorn.py,
test_gpu_sliced.py) share: a sample-only training term of cnf_ot_amd.applications, two times, against the float64
analytic adjoint of the flow pass (flow_adjoint_f64) seeded with the statistic's float64 restatement, and the same term
through ordinary autograd.  The caller passes its term, its autograd function, its restatement and its floor."""
import numpy as np
import torch

import flow_adjoint_f64 as fa

CONDS = np.array([0.3, 0.8], dtype=np.float32)
RNG_SEED = 77


def check(dev, tag, D, B, tgt, term, term_kw, auto, restate, floor, note=None, exact_autograd=False):
  """term: the applications function, called (model, D, params, tgt, CONDS, RNG_SEED, B, **term_kw[, grad=]);
  auto(x [S, B, D], y [S, M, D]) -> [S]: the autograd function with its constants bound;
  restate(samples [B, D] float64) -> (value, gradient in the samples [B, D], the run): the restatement against tgt;
  floor(samples [S, B, D] float64, the S float64 runs) -> the value's floor;
  note(float64 runs, float32 runs) -> text appended to the printed line;
  exact_autograd: the autograd route gives the fast path's gradient bit for bit (else: to S B 2^-24 of its largest
  entry, the float32 rounding of the final accumulation in two orders).
  Returns the autograd route's samples [S B, D] (detached) for what a caller checks beyond this."""
  from cnf_ot_amd import FlowConfig, FlowModel, Params, applications as app, autograd
  S = len(CONDS)
  cfg = FlowConfig(dim=D)
  params = Params.random(cfg, 0.2, seed=3 + D, device=dev)
  model = FlowModel(cfg)
  g = torch.zeros_like(params.flat)
  loss = term(model, D, params, tgt, CONDS, RNG_SEED, B, grad=g, **term_kw)
  plain = term(model, D, params, tgt, CONDS, RNG_SEED, B, **term_kw)
  v, gt = app.value_and_grad(lambda p, *a, **kw: term(model, D, p, *a, **kw))(params, tgt, CONDS, RNG_SEED, B, **term_kw)
  torch.cuda.synchronize()
  assert float(plain) == float(loss) == float(v) and torch.equal(gt.flat, g)
  # the float64 reference: the analytic adjoint of the flow pass, seeded with the restatement's gradient
  be = model.terms_backend(params)
  z = be.normal(RNG_SEED, B).cpu().numpy()
  zs, cs = np.tile(z, (S, 1)), np.repeat(CONDS, B)
  flat = params.flat.cpu().numpy()

  def ref(dt):
    out = fa.pass_vjp(cfg, flat, zs, cs, None, None, False, dt)[0]
    out = np.asarray(out, dtype=np.float64).reshape(S, B, D)
    vals, grads, runs = zip(*(restate(out[s]) for s in range(S)))
    ybar = np.concatenate(grads) / S
    return np.mean(vals), fa.pass_vjp(cfg, flat, zs, cs, ybar.astype(dt), None, False, dt)[3], out, runs
  v64, g64, out64, runs = ref(np.float64)
  v32, g32, _, runs32 = ref(np.float32)
  f_val = floor(out64, runs)
  e_v, e_g = abs(float(loss) - v64), float(np.abs(g.cpu().double().numpy() - g64).max())
  bound = fa.bound(g32, g64)
  print(f"\n[{tag}] loss {v64:.6f}: error {e_v:.2e} (float32 restatement {abs(v32 - v64):.2e}, floor "
        f"{f_val:.2e}) | gradient |.| {np.abs(g64).max():.3e}: error {e_g:.2e}, bound {bound:.2e}"
        + ("" if note is None else note(runs, runs32)))
  assert e_v <= 2.0 * abs(v32 - v64) + f_val
  assert e_g <= bound
  # the same term through ordinary autograd: flow_forward + the autograd function
  flat_t = params.flat.clone().requires_grad_(True)
  zt = torch.from_numpy(zs).to(dev)
  samples, _ = autograd.flow_forward(be, flat_t, zt, torch.from_numpy(CONDS).to(dev))
  val = auto(samples.view(S, B, D), torch.from_numpy(tgt).to(dev)[None].expand(S, -1, -1))
  assert val.shape == (S,) and val.dtype == torch.float64
  (val.sum() / S).backward()
  e_auto = float((flat_t.grad - g).abs().max())
  same = float(val.detach().sum() / S) == float(loss)
  print(f"[{tag}] autograd against the fast path: {e_auto:.2e}" + ("" if exact_autograd else f", values equal: {same}"))
  assert same
  if exact_autograd:
    assert torch.equal(flat_t.grad, g)
  else:
    assert e_auto <= S * B * 2.0 ** -24 * float(g.abs().max())
  return samples.detach()
