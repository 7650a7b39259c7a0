"""The power kind of the fused interaction energy on the GPU (softened power laws and the log kernel): cnf_interaction /
utils.interaction_energy / utils.interaction_field / applications.interaction_loss_fn / ot_loss_fn's `interaction=`,
against the float64 restatement (tests/interaction_power_ref.py) under test_gpu_interaction.py's bar with its EPS = 5e-6,
  e_fused <= 2 e_composed + floor,   floor = 4 EPS k_max (sums / (rows n) and pot),  4 EPS tau (force, max-norm),
e_composed the error of the same sums composed in NumPy float32 throughout, and k_max = sum_b max |W_b|, tau = sum_b
max |W_b'| over the pairs counted (the other kinds' scales are these maxima in closed form; a power law has none).  What
the kind adds per term to that bar's derivation: t_b = exp2(q_b log2 u), whose relative error is |q_b log2 u| ln 2 times
the rounding of the product and of v_log_f32 (2^-24 each): at the largest |q log2 u| of these specs and clouds (q = 1, u
< 2^9) 4e-7 of the term, below the 5e-7 per-term share the bar allows.

Shapes: N in {2, 63, 64, 65, 511, 512, 513, 1025} (the tile of 64 columns, the 512 rows of a workgroup, the first split,
a second row group), self mode and query mode with Q in {1, 130, 513}, D in {1, 2, 3, 10, 14}; specs with 1, 2, 3 and 4
terms: the log kernel, a repulsive Coulomb-like kernel (pw = 2 - D at D = 3, -1 elsewhere), an attractive-repulsive pair,
pw = 2 without softening (the quadratic kind restated), three and four mixed terms with a log term.

Every test prints its figures (run with -s); the largest e_fused / (2 e_composed + floor) per spec is printed by the
last test of the file and recorded in DESIGN.md 5.3p.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import interaction_power_ref as pr
import interaction_ref as ir

EPS = 5e-6                                   # test_gpu_interaction.py's, derived there
SELF = [(1, 2), (2, 63), (2, 64), (2, 65), (3, 511), (2, 512), (2, 513), (3, 1025), (10, 65), (14, 513)]      # (D, N)
QUERY = [(3, 1, 64), (2, 130, 513), (10, 513, 65), (14, 130, 1025), (1, 513, 2)]                              # (D, Q, N)
SHAPES = [(D, 0, N) for D, N in SELF] + QUERY
SHARE = {}


def _specs(D):
  return {"log": pr.spec([0.0], [1.0], 0.1),
          "coulomb": pr.spec([2.0 - D if D == 3 else -1.0], [-1.0], 0.1),
          "attractive-repulsive": pr.spec([4.0, 1.0], [1.0, -1.0], 0.05),
          "p2": pr.spec([2.0], [0.75], 0.0),
          "mixed/3": pr.spec([3.0, 0.0, -1.0], [0.5, 1.0, -0.25], 0.1),
          "mixed/4": pr.spec([4.0, 1.0, 0.0, -1.0], [0.5, -1.0, 0.75, -0.25], 0.2)}


SPEC_NAMES = list(_specs(1))


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def _inputs(D, Q, N, index, S=None):
  x = ir.cloud(D, N, 7000 + index, scale=1.0 + 0.125 * (index % 5), S=S)
  q = None if Q == 0 else (ir.cloud(D, Q, 8000 + index, scale=1.5, S=S) + np.float32(0.2)).astype(np.float32)
  return x, q


def _case(x, q, sp):
  """(pot, force, sum, k_max, tau) of the restatement and (pot, force, sum) of the float32 composition"""
  pot, force, total, _ = pr.rows(x, sp, q)
  k_max, tau, _ = pr.scales(x, sp, q)
  return (pot, force, total, k_max, tau), pr.rows(x, sp, q, dtype=np.float32)[:3]


@functools.lru_cache(maxsize=None)
def _reference(D, Q, N, index, name):
  x, q = _inputs(D, Q, N, index)
  return _case(x, q, _specs(D)[name])


def _call(dev, x, q, sp, want_pot=True, want_force=True, fill=None, stream=None, out=None):
  """test_gpu_interaction.py's: cnf_interaction through the C ABI on device tensors"""
  from cnf_ot_amd import _capi, utils
  from cnf_ot_amd.flows import _stream_ptr
  spec = utils.interaction_spec(**pr.kwargs(sp))
  S, N, D = x.shape
  Q = 0 if q is None else q.shape[1]
  rows = Q or N
  lib = _capi.lib()
  nbytes = ctypes.c_int64(0)
  _capi.check(lib.cnf_interaction_workspace(S, N, Q, D, int(want_force), ctypes.byref(nbytes)), "cnf_interaction_workspace")
  if out is None:
    ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
    if fill is not None:
      ws.fill_(fill)
    sums = torch.empty(S, dtype=torch.float64, device=dev)
    pot = torch.empty(S, rows, dtype=torch.float32, device=dev) if want_pot else None
    force = torch.empty(S, rows, D, dtype=torch.float32, device=dev) if want_force else None
  else:
    sums, pot, force, ws = out
  assert x.is_contiguous() and x.dtype == torch.float32 and (q is None or (q.is_contiguous() and q.dtype == torch.float32))
  ptr = lambda t: None if t is None else t.data_ptr()
  _capi.check(lib.cnf_interaction(ctypes.byref(spec), S, x.data_ptr(), N, ptr(q), Q, D, sums.data_ptr(), ptr(pot), ptr(force),
                                  ws.data_ptr(), nbytes.value, _stream_ptr(dev) if stream is None else stream),
              "cnf_interaction")
  if out is None:
    torch.cuda.synchronize()
  return sums, pot, force, ws


def _check(dev, x, q, sp, name, ref, comp, tag, got=None):
  xd = torch.from_numpy(x).to(dev)
  qd = None if q is None else torch.from_numpy(q).to(dev)
  if got is None:
    q1 = None if qd is None else qd[None]
    sums, pot, force, _ = _call(dev, xd[None], q1, sp)
    for wp, wf in ((False, False), (True, False), (False, True)):      # sums does not depend on what else is asked for
      s2, p2, f2, _ = _call(dev, xd[None], q1, sp, want_pot=wp, want_force=wf)
      assert torch.equal(sums, s2) and (p2 is None or torch.equal(p2, pot)) and (f2 is None or torch.equal(f2, force))
    got = (sums[0], pot[0], force[0])
  ref_pot, ref_force, ref_sum, k_max, tau = ref
  comp_pot, comp_force, comp_sum = comp
  rows, n = len(ref_pot), (len(x) - 1 if q is None else len(x))
  got_pot, got_force = got[1].cpu().double().numpy(), got[2].cpu().double().numpy()
  norm = float(rows) * n
  e = {"sum": (abs(float(got[0]) - ref_sum) / norm, abs(comp_sum - ref_sum) / norm, 4.0 * EPS * k_max),
       "pot": (float(np.abs(got_pot - ref_pot).max()), float(np.abs(comp_pot - ref_pot).max()), 4.0 * EPS * k_max),
       "force": (float(np.abs(got_force - ref_force).max()), float(np.abs(comp_force - ref_force).max()), 4.0 * EPS * tau)}
  share = max(a / (2.0 * b + c) for a, b, c in e.values())
  SHARE[name] = max(SHARE.get(name, 0.0), share)
  print(f"\n[interaction power {tag}] mean {ref_sum / norm:.6f} k_max {k_max:.3g} tau {tau:.3g} | " + " | ".join(
    f"{k}: fused {a:.2e} composed {b:.2e} floor {c:.2e}" for k, (a, b, c) in e.items()) + f" | share {share:.4f}")
  assert np.isfinite(float(got[0])) and np.isfinite(got_pot).all() and np.isfinite(got_force).all()
  for k, (a, b, c) in e.items():
    assert a <= 2.0 * b + c, (tag, k, a, b, c)
  return got_pot, got_force


@pytest.mark.parametrize("name", SPEC_NAMES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "D%d-Q%d-N%d" % s)
def test_value_field_and_force_against_the_restatement(dev, shape, name):
  D, Q, N = shape
  index = SHAPES.index(shape)
  x, q = _inputs(D, Q, N, index)
  ref, comp = _reference(D, Q, N, index, name)
  _check(dev, x, q, _specs(D)[name], name, ref, comp, f"{name} D={D} Q={Q} N={N}")


@pytest.mark.parametrize("name", SPEC_NAMES)
def test_three_sets_with_their_own_data(dev, name):
  D, N, Q, S = 2, 257, 130, 3
  x, q = _inputs(D, Q, N, 40, S=S)
  x[1] *= np.float32(1.25)                               # (the sets differ in law as well as in draw)
  x[2] += np.float32(0.5)
  sp = _specs(D)[name]
  xd, qd = torch.from_numpy(x).to(dev), torch.from_numpy(q).to(dev)
  for mode, qq in (("self", None), ("query", qd)):
    sums, pot, force, _ = _call(dev, xd, qq, sp)
    for s in range(S):
      qs = None if qq is None else q[s]
      ref, comp = _case(x[s], qs, sp)
      _check(dev, x[s], qs, sp, name, ref, comp, f"S=3 set {s} {mode} {name}", got=(sums[s], pot[s], force[s]))
    assert len({round(float(v) / (N * N), 5) for v in sums}) == S           # three different numbers: no set read twice


COINCIDENT = {"log": pr.spec([0.0], [1.0], 0.1), "mixed/4": pr.spec([4.0, 1.0, 0.0, -1.0], [0.5, -1.0, 0.75, -0.25], 0.2),
              "p2, eps 0": pr.spec([2.0], [0.75], 0.0), "p4, eps 0": pr.spec([4.0], [0.5], 0.0),
              "p2 + p4, eps 0": pr.spec([2.0, 4.0], [0.75, -0.25], 0.0)}


@pytest.mark.parametrize("name", list(COINCIDENT))
def test_coincident_pairs(dev, name):
  D, N = 3, 700
  sp = COINCIDENT[name]
  x, _ = _inputs(D, 0, N, 44)
  x[600:620] = x[:20]                                     # (another workgroup's rows and another split's columns)
  ref, comp = _case(x, None, sp)
  _, force = _check(dev, x, None, sp, name, ref, comp, f"{name}, duplicated rows")
  assert np.array_equal(force[600:620], force[:20])       # equal points, equal forces: their own pair adds exactly 0
  # query mode with every query equal to a source
  q = x[590:610].copy()
  ref, comp = _case(x, q, sp)
  _check(dev, x, q, sp, name, ref, comp, f"{name}, queries equal to sources")
  # nothing but coincident pairs: the force is exactly 0 and the value W(0)
  same = np.repeat(x[:1], 70, axis=0)
  for qq in (None, same[:5].copy()):
    sums, pot, f, _ = _call(dev, torch.from_numpy(same).to(dev)[None], None if qq is None else torch.from_numpy(qq).to(dev)[None], sp)
    assert torch.isfinite(sums).all() and torch.isfinite(pot).all() and not f.any()
    w0 = float(pr.kernel(np.zeros((1, 1, D)), sp)[0][0, 0]) if sp["eps"] > 0.0 else 0.0
    # (eps = 0: the kernel evaluates the pair at u = 1e-30, its clamp, where |W| <= 1e-30 sum_b |amp_b / pw_b|)
    assert float((pot.double() - w0).abs().max()) <= 4.0 * EPS * abs(w0) + 1e-30 * sum(abs(a) for a in sp["amp"])


def test_p_2_without_softening_against_the_quadratic_kind(dev):
  D, N, amp = 2, 600, 0.75
  x, _ = _inputs(D, 0, N, 45)
  sp, quad = pr.spec([2.0], [amp], 0.0), ir.spec("quadratic", [amp])
  xd = torch.from_numpy(x).to(dev)[None]
  ref, comp = _case(x, None, sp)
  _check(dev, x, None, sp, "p2", ref, comp, "p = 2, eps = 0")
  a, b = _call(dev, xd, None, sp), _call(dev, xd, None, quad)
  k_max, tau = ir.k_max(x, quad), ir.tau(x, quad)
  e_sum = abs(float(a[0][0] - b[0][0])) / (N * (N - 1.0))
  e_pot, e_force = float((a[1].double() - b[1].double()).abs().max()), float((a[2].double() - b[2].double()).abs().max())
  print(f"[power p = 2 against the quadratic kind] sum {e_sum:.2e} pot {e_pot:.2e} (floor {4 * EPS * k_max:.2e}) force {e_force:.2e} "
        f"(floor {4 * EPS * tau:.2e})")
  # the bar itself, with the quadratic kind's scales: e <= 2 e_composed + floor
  e_c = [abs(comp[2] - ref[2]) / (N * (N - 1.0)), float(np.abs(comp[0] - ref[0]).max()), float(np.abs(comp[1] - ref[1]).max())]
  assert e_sum <= 2 * e_c[0] + 4 * EPS * k_max and e_pot <= 2 * e_c[1] + 4 * EPS * k_max
  assert e_force <= 2 * e_c[2] + 4 * EPS * tau


@pytest.mark.parametrize("name", ["log", "attractive-repulsive", "mixed/4"])
def test_reproducibility(dev, name):
  D, N, Q, S = 3, 700, 1100, 2
  x, q = _inputs(D, Q, N, 41, S=S)
  sp = _specs(D)[name]
  xd, qd = torch.from_numpy(x).to(dev), torch.from_numpy(q).to(dev)
  same = lambda a, b: all(torch.equal(u, v) for u, v in zip(a[:3], b[:3]))
  for qq in (None, qd):
    base = _call(dev, xd, qq, sp)
    assert same(base, _call(dev, xd, qq, sp))                          # two calls
    assert same(base, _call(dev, xd, qq, sp, fill=0xFF))               # (0xFF bytes: NaN doubles wherever a word is read unwritten)
    # one call replayed from a captured graph: a single stream, one linear chain of launches, nothing allocated
    replay = _call(dev, xd.flip(1).contiguous(), qq, sp)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
      _call(dev, xd, qq, sp, stream=side.cuda_stream, out=replay)
    for t in replay[:3]:
      t.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    assert same(base, replay)


@pytest.mark.parametrize("name", ["coulomb", "mixed/4"])
def test_the_python_surface(dev, name):
  from cnf_ot_amd import autograd, utils
  D, N, Q = 3, 257, 130
  x, q = _inputs(D, Q, N, 46)
  sp = _specs(D)[name]
  kw = pr.kwargs(sp)
  a = utils.interaction_energy(x, want_grad=True, want_field=True, **kw)
  xd, qd = torch.from_numpy(x).to(dev)[None], torch.from_numpy(q).to(dev)[None]
  sums, pot, force, _ = _call(dev, xd, None, sp)
  assert torch.equal(a["sums"], sums) and torch.equal(a["potential"], pot[0]) and torch.equal(a["grad"], force[0] * (1.0 / N))
  assert abs(float(a["energy"][0]) - pr.energy(x, sp)) <= 2.0 * EPS * pr.scales(x, sp)[0]
  f = utils.interaction_field(q, x, **kw)
  sq, pq, fq, _ = _call(dev, xd, qd, sp)
  assert torch.equal(f["sums"], sq) and torch.equal(f["potential"], pq[0]) and torch.equal(f["force"], fq[0])
  xt = xd[0].clone().requires_grad_(True)
  val = autograd.interaction_energy(xt, **kw)
  val.sum().backward()
  assert float(val.detach()[0]) == float(a["energy"][0]) and torch.equal(xt.grad, a["grad"])


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("name", ["log", "attractive-repulsive", "mixed/4"])
def test_training_term_against_the_float64_adjoint(dev, D, name):
  """test_gpu_interaction.py's check of interaction_loss_fn (the kernel as a cost), with the power kind"""
  import sample_term_check
  from cnf_ot_amd import applications as app, autograd
  B = 96
  sp = _specs(D)[name]
  kw = pr.kwargs(sp)
  none = np.zeros((1, D), dtype=np.float32)
  sample_term_check.check(
      dev, f"interaction_loss_fn D={D} power {name}", D, B, none,
      lambda model, dim, params, tgt, cond, rng, batch, **k: app.interaction_loss_fn(model, dim, params, cond, rng, batch, **k),
      kw, auto=lambda x, y: autograd.interaction_energy(x, **kw),
      restate=lambda out: (pr.energy(out, sp), pr.rows(out, sp)[1] / len(out), None),
      floor=lambda out64, runs: 2.0 * EPS * max(pr.scales(o, sp)[0] for o in out64))


@pytest.mark.parametrize("name", ["log", "attractive-repulsive"])
def test_ot_loss_gains_the_interaction_cost(dev, name):
  """test_gpu_interaction.py's test_composites_gain_the_interaction_part for ot "free", under its bounds"""
  from cnf_ot_amd import FlowConfig, FlowModel, Params, applications as app
  dim, batch, tbs, rng, strength, T = 2, 2048, 4, 11, 0.7, 1
  sub = batch // 32
  cfg = FlowConfig(dim=dim)
  params = Params.random(cfg, 0.2, seed=6, device=dev)
  model = FlowModel(cfg)
  kw = pr.kwargs(_specs(dim)[name])
  ot = lambda **k: app.ot_loss_fn(model, dim, 1, 0.01, tbs, "free", params, rng, 5000.0, batch, **k)
  g0, g1, gi = (torch.zeros_like(params.flat) for _ in range(3))
  base, full = ot(grad=g0), ot(grad=g1, interaction=(kw, strength))
  v, gv = app.value_and_grad(lambda p, *a, **k: app.ot_loss_fn(model, dim, 1, 0.01, tbs, "free", p, *a, **k))(
      params, rng, 5000.0, batch, interaction=(kw, strength))
  part = app.interaction_loss_fn(model, dim, params, app.draw_t_batch(rng, tbs, float(T)), rng, sub, grad=gi, **kw)
  torch.cuda.synchronize()
  assert float(v) == float(full) and torch.equal(gv.flat, g1)
  want = float(base) + strength * T * float(part)
  want_g = g0.double() + strength * T * gi.double()
  e_v, e_g = abs(float(full) - want), float((g1.double() - want_g).abs().max())
  bound = 2.0 ** -24 * (tbs * sub * strength * T * float(gi.abs().max()) + 4 * float(want_g.abs().max()))
  print(f"[ot free + power {name}] loss {float(base):.6f} + {strength * T * float(part):.6f}: error {e_v:.2e} | gradient "
        f"|.| {float(want_g.abs().max()):.3e}: error {e_g:.2e} (bound {bound:.2e})")
  assert e_v <= 2.0 ** -52 * abs(want) and e_g <= bound and float(part) != 0.0


@pytest.mark.parametrize("name", ["log", "attractive-repulsive"])
def test_ot_loss_with_the_cost_against_float64_finite_differences(dev, name):
  """value_and_grad of ot_loss_fn with the kernel as a cost, less the same call without it, against the float64
  restatement of the cost J = strength T mean_t F(flow(z, t)) on the cost's own samples (the first batch // 32 rows of the
  draw) and times: the value, the gradient entry by entry against flow_adjoint_f64's analytic adjoint, which central
  differences of J in float64 (step 1e-5 along three random unit directions) confirm first, and those directional
  derivatives themselves.  Bounds: test_gpu_interaction.py's for the composites (the float32 accumulation of the part's
  adjoints and of the loss's terms, 2^-24 of their magnitudes) plus flow_adjoint_f64.bound for the float32 pass of the
  part, as test_training_term_against_the_float64_adjoint holds it; _lambda = 0 keeps the loss's own gradient, whose
  rounding the difference carries, at the cost's scale."""
  import flow_adjoint_f64 as fa
  from cnf_ot_amd import FlowConfig, FlowModel, Params, applications as app
  dim, batch, tbs, rng, strength, T = 2, 2048, 4, 11, 0.7, 1
  sub = batch // 32
  cfg = FlowConfig(dim=dim)
  params = Params.random(cfg, 0.2, seed=6, device=dev)
  model = FlowModel(cfg)
  sp = _specs(dim)[name]
  kw = pr.kwargs(sp)
  vg = app.value_and_grad(lambda p, *a, **k: app.ot_loss_fn(model, dim, 1, 0.01, tbs, "free", p, *a, **k))
  v1, gr1 = vg(params, rng, 0.0, batch, interaction=(kw, strength))
  v0, gr0 = vg(params, rng, 0.0, batch)
  torch.cuda.synchronize()
  be = model.terms_backend(params)
  z = be.normal(rng, batch)[:sub].cpu().numpy()
  th = np.asarray(app._conds(app.draw_t_batch(rng, tbs, float(T))), dtype=np.float32)
  S = len(th)
  zs, cs = np.tile(z, (S, 1)), np.repeat(th, sub)
  flat = params.flat.cpu().double().numpy()
  c = strength * T

  def J(fl, dt=np.float64, grad=False):
    out = np.asarray(fa.pass_vjp(cfg, fl, zs, cs, None, None, False, dt)[0], dtype=np.float64).reshape(S, sub, dim)
    val = c * float(np.mean([pr.energy(o, sp) for o in out]))
    if not grad:
      return val
    ybar = c * np.concatenate([pr.rows(o, sp)[1] / sub for o in out]) / S
    return val, np.asarray(fa.pass_vjp(cfg, fl, zs, cs, ybar.astype(dt), None, False, dt)[3], dtype=np.float64), out
  (J64, g64, out64), (J32, g32, _) = J(flat, grad=True), J(flat, np.float32, grad=True)
  got_v, got_g = float(v1) - float(v0), gr1.flat.cpu().double().numpy() - gr0.flat.cpu().double().numpy()
  big = max(float(gr1.flat.abs().max()), float(gr0.flat.abs().max()))
  per_entry = 2.0 ** -24 * (tbs * sub * float(np.abs(g64).max()) + 2 * 4 * big) + fa.bound(g32, g64)
  f_val = c * 2.0 * EPS * max(pr.scales(o, sp)[0] for o in out64) + 2.0 ** -50 * max(abs(float(v1)), abs(float(v0)))
  e_v, e_g = abs(got_v - J64), float(np.abs(got_g - g64).max())
  print(f"\n[ot free + power {name}, value_and_grad] cost {J64:.6f}: error {e_v:.2e} (float32 restatement {abs(J32 - J64):.2e}, floor "
        f"{f_val:.2e}) | gradient |.| {np.abs(g64).max():.3e}: error {e_g:.2e}, bound {per_entry:.2e}")
  assert J64 != 0.0 and e_v <= 2.0 * abs(J32 - J64) + f_val
  assert e_g <= per_entry
  gen = np.random.default_rng(3)
  for k in range(3):
    v = gen.standard_normal(flat.size)
    v /= np.linalg.norm(v)
    h = 1e-5
    dd = (J(flat + h * v) - J(flat - h * v)) / (2.0 * h)
    # central differences in float64: truncation h^2 / 6 of the third derivative, rounding 2^-52 |J| / h
    e_ref, e_dir = abs(float(g64 @ v) - dd), abs(float(got_g @ v) - dd)
    print(f"[ot free + power {name}] direction {k}: finite difference {dd:.8e}, analytic float64 {float(g64 @ v):.8e} (apart "
          f"{e_ref:.1e}), value_and_grad {float(got_g @ v):.8e} (apart {e_dir:.1e}, bound {per_entry * np.abs(v).sum():.1e})")
    assert e_ref <= 1e-7 * max(abs(dd), float(np.abs(g64).max()))
    assert e_dir <= per_entry * float(np.abs(v).sum()) + 1e-7 * abs(dd)


def test_share_of_the_bound_per_spec(dev):
  """(runs after the cases above in file order: prints what they recorded)"""
  for name, share in SHARE.items():
    print(f"[interaction power] {name}: largest e_fused / (2 e_composed + floor) = {share:.4f}")
    assert share <= 1.0
