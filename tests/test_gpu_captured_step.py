"""solvers.CapturedUpdate BETWEEN its replays -- what the bit-for-bit test of test_gpu_grad.py (ten uninterrupted steps
from a fresh optimiser on a model nothing else touches) does not run: eager losses on the same engine between two
replays (the caches whose tensors the graph reads by address), model.apply.* after a replay with
assume_unchanged_params, and an optimiser state that is handed over at step 5.

The kernels are covered elsewhere; these tests hold the HOST layer to what it hands them: live addresses, the current
parameters, the right step count.  References: the very same body run eagerly (bit for bit), a fresh engine (bit for
bit), the float64 oracle at test_gpu_parity.py's bar, and step_kernels_ref.adam_ref at the rounding bounds of
step_kernels_ref.adam_bounds (the bounds test_gpu_step_kernels.py holds cnf_adam_step_dev to)."""
import gc
import itertools
import weakref

import numpy as np
import pytest
import torch

import oracle
import step_kernels_ref as sk
from test_gpu_parity import TOL_LP_DATA_MAX, _err      # fp32 log_prob against the oracle at dim 2: 1e-5 absolute

pytestmark = pytest.mark.gpu
LAMBDA = 5000.0
_TAG = itertools.count(1)      # a run's own weight patterns: a pattern another run has left in _WEIGHTS inserts nothing


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def _start(dev, batch=2048, lr=1e-3):
  """(config, model, params): ot at dim 2, two times per step; model.init(7) plus the seeded perturbation of
  test_captured_step_equals_the_eager_step_bit_for_bit"""
  from cnf_ot_amd import solvers
  config = solvers.load_config(overrides={"general": {"type": "ot", "dim": 2, "t_batch_size": 2},
                                          "train": {"batch_size": batch, "lr": lr}})
  model = solvers.build_model(config)
  params = model.init(7)
  params.flat.add_(0.05 * torch.randn(params.flat.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1)))
  return config, model, params


def _interrupted_run(dev, replay, table, monkeypatch):
  """A1's script for one CapturedUpdate.  Returns (parameters, mu, nu, the eight losses)."""
  from cnf_ot_amd import solvers, applications as app
  B = 16384 if table else 2048
  config, model, params = _start(dev, B)
  eng = model.engine(dev)
  loss_fn = solvers.bind_loss(config, model)
  vg = app.value_and_grad(loss_fn)
  opt = solvers.Adam(1e-3)
  st = opt.init(params)
  upd = solvers.CapturedUpdate(loss_fn, opt, B, replay=replay)
  fused = []      # cnf_kinetic_potential_vjp calls that were taken, per phase
  if table:
    eng.set_pwl(2)
    orig = eng.kinetic_potential_vjp
    monkeypatch.setattr(eng, "kinetic_potential_vjp", lambda *a, **k: (lambda r: (fused.append(r is not None), r)[1])(orig(*a, **k)))
  try:
    # 1. the cached uploads ([0], [T]), the weight vector and (table route) _kp_work come to exist on the CALLER's stream
    if table:
      vg(params, 5, LAMBDA, B)
      assert fused == [True] and getattr(eng, "_kp_work", None) is not None
    else:
      loss_fn(params, 5, LAMBDA, B)
    # 2. two warm-up calls, the capture, one replay
    losses, refs = [], None
    for step in range(4):
      loss, params, st = upd(params, 1000 + 17 * step, LAMBDA, st)
      losses.append(loss.clone())
      if step == upd.WARMUP and replay:      # right after the capture call: what the graph reads and does not own
        assert upd.graph is not None
        held = list(eng._cond_cache.values()) + list(app._WEIGHTS.values()) + [getattr(eng, "_kp_work", None)]
        refs = [weakref.ref(t) for t in held if t is not None]
        assert len(refs) >= (4 if table else 3)
        del held
    if table:
      assert len(fused) == 1 + (4 if not replay else upd.WARMUP + 1) and all(fused)      # inside the step, the capture included
    # 3. eager work on the same engine: new time batches fill _cond_cache (32 keys), new patterns _WEIGHTS (64 keys)
    for k in range(16):
      loss_fn(params, 100 + k, LAMBDA, B)
    for k in range(16):      # (one new key per evaluation off the table route: sixteen more reach the 32)
      vg(params, 200 + k, LAMBDA, 2 * B if (table and k == 0) else B)      # table: a larger call replaces _kp_work
    ctx = app._Ctx(model, params, 0, None)
    tag = 1000.0 * next(_TAG)
    for n in (1, 2, 3, 4):
      flat = torch.ones(n, dtype=torch.float64, device=dev)
      for j in range(17):
        ctx.weighted(flat, [flat], [tag + j])
    del ctx
    # 4. the blocks a cache gave up go to the next allocations of that size on this stream: NaN where the graph reads
    n_work = eng._kp_work.numel() if table else 0
    pressure = [torch.full((128 * (1 + i % 8),), float("nan"), dtype=torch.float32, device=dev) for i in range(400)]
    pressure += [torch.full((n,), float("nan"), dtype=torch.float32, device=dev) for n in (n_work, n_work // 2) if n]
    torch.cuda.synchronize()
    gc.collect()
    if refs is not None:
      # the script did evict: none of the tensors the graph reads is still its cache's entry ...
      cached = {id(t) for t in eng._cond_cache.values()} | {id(t) for t in app._WEIGHTS.values()} | {id(getattr(eng, "_kp_work", None))}
      assert not any(id(r()) in cached for r in refs if r() is not None)
      # ... and every one of them is still alive (asserted BEFORE the next replay: none runs on memory known to be freed)
      dead = sum(r() is None for r in refs)
      assert dead == 0, f"{dead} of {len(refs)} tensors the graph reads by address were freed between two replays"
    # 5. four more calls
    for step in range(4, 8):
      loss, params, st = upd(params, 1000 + 17 * step, LAMBDA, st)
      losses.append(loss.clone())
    torch.cuda.synchronize()
    assert (upd.graph is not None) == replay and st.step == 8
    del pressure
    return params.flat.clone(), st.mu.clone(), st.nu.clone(), torch.stack(losses)
  finally:
    if table:
      eng.set_pwl(1)


@pytest.mark.parametrize("table", [False, True], ids=["fused", "table"])
def test_replays_survive_eager_work_on_the_same_engine(dev, table, monkeypatch):
  """Between the replay of call 4 and call 5: 32 eager evaluations of the bound loss with new integer keys (16 values, 16
  value_and_grad; each uploads a new time batch into FlowEngine._cond_cache, emptied at 32 keys), 68 new weight
  patterns through _Ctx.weighted (applications._WEIGHTS, emptied at 64), on the table route (set_pwl(2), batch 16384,
  the kinetic term through cnf_kinetic_potential_vjp: counted) one evaluation at twice the batch, which replaces
  _kp_work; then 400 NaN-filled tensors of 512 B to 4 KB and one of _kp_work's size take the freed blocks.
  Asserted: the tensors the graph reads by address -- every _cond_cache and _WEIGHTS value and _kp_work as they stood
  right after the capture call -- have left their caches and are all still alive; then parameters, both moments and
  all eight losses of the replayed run are the BITS of the same script with replay=False, and every loss is finite.
  The liveness assertion stands before call 5 on purpose: where it fails, no replay runs on freed memory.
  Measured: 9 (fused) and 11 (table) such tensors; before CapturedUpdate kept them, all 9 and all 11 were freed here."""
  res = [_interrupted_run(dev, replay, table, monkeypatch) for replay in (False, True)]
  for a, b in zip(res[0], res[1]):
    assert torch.equal(a, b)
  assert torch.isfinite(res[0][3]).all() and torch.isfinite(res[1][3]).all()


def test_engine_after_a_replay_holds_the_current_parameters(dev):
  """FlowModel(assume_unchanged_params=True) during captured training: after the capture call and after each of two
  pure replays, model.apply.log_prob at 4099 fixed points (one partial wave), cond 0.4, is the BITS of a fresh engine
  loaded with the current parameters, and within test_gpu_parity.py's 1e-5 of the float64 oracle at those parameters --
  which the oracle at the parameters of the call before misses by more than ten times that (the graph loads the
  parameters first and updates them last: an engine that skips its reload is one step behind).
  Measured at lr 1e-3, after calls 3, 4, 5: the oracle's gap between consecutive parameters 8.9e-1, 7.4e-1, 6.3e-1 (the
  bar asks for 1e-4; the tail points move most), the error against the oracle 3.2e-7, 2.3e-7, 3.4e-7.  Without
  mark_updated after each replay the call-4 value is the previous parameters': 7.4e-1 off."""
  from cnf_ot_amd import solvers, FlowEngine
  config, model, params = _start(dev)
  model.assume_unchanged_params = True
  opt = solvers.Adam(1e-3)
  st = opt.init(params)
  upd = solvers.CapturedUpdate(solvers.bind_loss(config, model), opt, 2048, replay=True)
  x = 1.5 * torch.randn(4099, 2, generator=torch.Generator().manual_seed(3))
  x64, c64 = x.double().numpy(), [float(np.float32(0.4))]
  x, cond = x.to(dev), torch.tensor([0.4], device=dev)
  ocfg = oracle.OracleConfig(D=2)
  model.apply.log_prob(params, x, cond)      # (the engine has loaded this very tensor before the first step)
  for call in range(5):
    before = params.flat.cpu().double().numpy()
    _, params, st = upd(params, 1000 + 17 * call, LAMBDA, st)
    if call < upd.WARMUP:
      continue
    assert upd.graph is not None
    lp = model.apply.log_prob(params, x, cond)
    fresh = FlowEngine(model.cfg, dev).load(params).log_prob(x, cond)
    now = params.flat.cpu().double().numpy()
    want, stale = oracle.log_prob(ocfg, now, x64, c64), oracle.log_prob(ocfg, before, x64, c64)
    err, gap = _err(lp, want).max(), np.abs(stale - want).max()
    print(f"\n[log_prob after call {call + 1}] err vs the oracle {err:.2e}; oracle gap to the previous parameters {gap:.2e}")
    assert gap > 10 * TOL_LP_DATA_MAX
    assert torch.equal(lp, fresh)
    assert err <= TOL_LP_DATA_MAX


def test_captured_step_continues_an_optimiser_state(dev):
  """An AdamState at step 5 (five eager steps) handed to CapturedUpdate, four calls: the replayed run is the eager body's
  BITS; opt_state.step is 9; per call, parameters and both moments are adam_ref(before, the call's own gradient,
  step = 6, 7, 8, 9) within step_kernels_ref.adam_bounds; the first call's parameters are OUTSIDE those bounds around
  adam_ref(step = 1), the count a fresh device state would give.  A state stepped elsewhere is refused.
  Measured, eager and replayed alike: worst error / bound over the four calls p 0.794, mu 0.534, nu 0.476; the first
  call's parameters are 7.8e3 bounds away from adam_ref(step = 1).  With the device count starting at 0 whatever the
  state's step, the first call's parameters were 8.5e4 bounds off adam_ref(step = 6)."""
  from cnf_ot_amd import solvers, Params
  config, model, params = _start(dev)
  loss_fn = solvers.bind_loss(config, model)
  lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
  opt = solvers.Adam(lr)
  st = opt.init(params)
  eager = solvers.make_update(loss_fn, opt, 2048, capture=False)
  for i in range(5):
    _, params, st = eager(params, 500 + i, LAMBDA, st)
  assert st.step == 5 and (opt.b1, opt.b2, opt.eps) == (b1, b2, eps)
  host = lambda t: t.detach().cpu().numpy().copy()
  res, worst = [], np.zeros(3)
  for replay in (False, True):
    p = Params(params.cfg, params.flat.clone())
    s = solvers.AdamState(st.step, st.mu.clone(), st.nu.clone())
    upd = solvers.CapturedUpdate(loss_fn, opt, 2048, replay=replay)
    seen, vg = [], upd.vg
    upd.vg = lambda *a, _vg=vg, _seen=seen, **k: (lambda r: (_seen.append(r[1]), r)[1])(_vg(*a, **k))
    losses = []
    for i in range(1, 5):
      before = [host(t) for t in (p.flat, s.mu, s.nu)]
      loss, p, s = upd(p, 2000 + 17 * i, LAMBDA, s)
      torch.cuda.synchronize()
      losses.append(loss.clone())
      g = host(seen[-1].flat)      # (replayed: the tensor the graph writes, read after the replay)
      got = [host(t) for t in (p.flat, s.mu, s.nu)]
      want, bounds, _ = sk.adam_bounds(before[0], g, before[1], before[2], lr, b1, b2, eps, 5 + i)
      errs = [np.abs(a.astype(np.float64) - w) for a, w in zip(got, want)]
      ratios = [sk.worst_ratio(e, b) for e, b in zip(errs, bounds)]
      worst = np.maximum(worst, ratios)
      print(f"\n[{'replayed' if replay else 'eager'} call {i}: step {5 + i}] worst err / bound: p {ratios[0]:.3f} mu {ratios[1]:.3f} nu {ratios[2]:.3f}")
      assert all((e <= b).all() for e, b in zip(errs, bounds))
      if i == 1:
        want1, bounds1, _ = sk.adam_bounds(before[0], g, before[1], before[2], lr, b1, b2, eps, 1)
        r1 = sk.worst_ratio(np.abs(got[0].astype(np.float64) - want1[0]), bounds1[0])
        print(f"[first call against step = 1] worst err / bound: p {r1:.3g}")
        assert r1 > 1.0
    assert s.step == 9 and (upd.graph is not None) == replay and len(seen) == (3 if replay else 4)
    res.append((p.flat.clone(), s.mu.clone(), s.nu.clone(), torch.stack(losses)))
    s.step += 1      # stepped elsewhere in between
    with pytest.raises(ValueError, match="stepped elsewhere"):
      upd(p, 1, LAMBDA, s)
  print(f"[worst over both runs] p {worst[0]:.3f} mu {worst[1]:.3f} nu {worst[2]:.3f}")
  for a, b in zip(res[0], res[1]):
    assert torch.equal(a, b)
  assert torch.isfinite(res[0][3]).all()
