"""The fused interaction energy on the GPU: cnf_interaction / utils.interaction_energy / utils.interaction_field /
autograd.interaction_energy / applications.interaction_loss_fn / the composites' `interaction=` /
solvers.evaluate_interaction, against the float64 restatement (tests/interaction_ref.py), with the torch float32
composition of the same sums -- direct differences, pair matrices reduced in float64 -- as the yardstick for the fused
error, test_gpu_mmd.py's:
  e_fused <= 2 e_composed + floor,   floor = 4 EPS k_max (sums / (rows n) and pot),  4 EPS tau (force, max-norm),
EPS = 5e-6: the kernel's float32 accumulators live for one tile of IA_TILE = 64 columns, so a partial sum errs by at most
64 * 2^-24 = 3.8e-6 relative to the tile's largest term times its length, and per-term rounding (the difference, the
fmaf chain of the distance, one v_exp_f32 -- max a e^-a = 0.37 bounds the effect of the argument's rounding -- and the
fmaf with the amplitude) stays below 5e-7 k_max; the doubles above the tiles add nothing at this level.  k_max = sum_b
|amp_b| (Gaussian, exponential) or |amp_0| max d^2 / 2 of the restatement (quadratic); tau = sum_b |amp_b| 0.61 / bw_b
(Gaussian), sum_b |amp_b| / bw_b (exponential), |amp_0| times the largest pair distance (quadratic).  The energy
F = sums / (2 N (N - 1)) is half a pair mean: its floor is 2 EPS k_max.

The kernel's own boundaries, each with a shape below, at and above it (BOUNDARY_SELF, BOUNDARY_QUERY): IA_ROWS = 512 rows
per workgroup (N or Q = 511, 512, 513), IA_TILE = 64 columns per tile (N = 63, 64, 65), and the column split, which
exceeds 1 from the first shape whose sources leave one tile: N = 65 for one set (cnf_interaction_splits, asserted below).

Measured on one MI355X (every test prints its figures: run with -s), errors against the restatement, fused / composed,
largest over the 18 shapes of a kernel:
  Gaussian, 1 term        pair mean 3.2e-8 / 3.2e-8   pot 2.2e-7 / 3.2e-8   force 8.3e-8 / 3.0e-8   (at most 0.011 of the floor)
  Gaussian, 4 signed      pair mean 6.4e-8 / 3.4e-8   pot 2.3e-7 / 3.4e-8   force 6.2e-8 / 6.2e-8   (0.005)
  Morse                   pair mean 9.2e-9 / 4.1e-9   pot 5.2e-8 / 4.1e-9   force 2.5e-8 / 8.4e-8   (0.002)
  quadratic (means 2-23)  pair mean 1.6e-7 / 1.3e-8   pot 6.4e-6 / 3.2e-7   force 8.9e-7 / 6.8e-8   (0.007)
  D=2 N=5000 Gaussian x 4 pair mean 2.3e-10 / 1.4e-9  pot 5.7e-8 / 1.1e-8   force 1.3e-8 / 8.8e-9
  D=14 N=129 quadratic    pair mean 1.6e-7 / 1.3e-8   pot 6.3e-6 / 3.2e-7   force 8.1e-7 / 2.8e-8   (floors 1.5e-3, 2.1e-4)
  interaction_loss_fn, D = 2 / 3   loss 4.0e-9 / 3.0e-9 (Gaussian x 4), 6.6e-10 / 6.8e-10 (Morse), 2.3e-8 / 3.6e-7 (quadratic);
                          parameter gradient 8.3e-9 / 2.0e-8, 5.7e-9 / 1.4e-8, 2.2e-7 / 4.3e-7 against flow_adjoint_f64.bound =
                          1.3e-7 / 4.1e-7, 3.9e-8 / 2.8e-7, 7.7e-6 / 5.9e-6; autograd.interaction_energy(flow_forward(...))
                          gave the fast path's value and gradient bit for bit
  composites              value: the one float64 addition exactly (error 0); gradient 1.6e-3 .. 3.5e-3 at |g| 3.7e4 .. 8.3e4
                          against bounds of 1.1e-2 .. 2.5e-2
  60 Adam steps           loss 0.9487 -> 0.0914, tr cov at t = 0.5 1.8937 -> 0.1825
  evaluate_interaction    quadratic: energy and amp tr(cov) / 2 within 5.1e-9 (floor 4.7e-4; Monte-Carlo level 3e-2 .. 5e-2)
More: profiles/interaction/README.md.
"""
import ctypes
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import interaction_ref as ir

EPS = 5e-6
SELF_SHAPES = [(1, 2), (2, 65), (3, 257), (10, 300), (14, 129), (2, 5000)]                  # (D, N)
QUERY_SHAPES = [(3, 1, 64), (2, 130, 257), (10, 257, 300)]                                  # (D, Q, N)
BOUNDARY_SELF = [(2, 63), (2, 64), (2, 511), (2, 512), (2, 513), (3, 1025)]                 # ((2, 65) is above)
BOUNDARY_QUERY = [(2, 511, 63), (2, 512, 64), (2, 513, 65)]
SHAPES = [(D, 0, N) for D, N in SELF_SHAPES + BOUNDARY_SELF] + QUERY_SHAPES + BOUNDARY_QUERY  # (D, Q or 0, N)


def _f32(v):
  return [float(np.float32(a)) for a in v]      # (as the kernel receives them)


def _specs(D):
  r = math.sqrt(D)
  return {"gaussian/1": ir.spec("gaussian", [1.0], _f32([r])),
          "gaussian/4": ir.spec("gaussian", [1.0, -0.5, 0.25, -0.75], _f32([0.5 * r, r, 2.0 * r, 4.0 * r])),
          "morse": ir.spec("exponential", [1.0, -0.5], [0.5, 2.0]),
          "quadratic": ir.spec("quadratic", [0.75])}


SPEC_NAMES = list(_specs(1))


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def _inputs(D, Q, N, index, S=None):
  """(x [N, D], q [Q, D] or None) -- [S, ., D] with S"""
  x = ir.cloud(D, N, 2000 + index, scale=1.0 + 0.125 * (index % 5), S=S)
  q = None if Q == 0 else (ir.cloud(D, Q, 3000 + index, scale=1.5, S=S) + np.float32(0.2)).astype(np.float32)
  return x, q


@functools.lru_cache(maxsize=None)
def _reference(D, Q, N, index, name):
  """The restatement of one (shape, spec) case, computed once: (pot, force, sum, k_max, tau)"""
  x, q = _inputs(D, Q, N, index)
  sp = _specs(D)[name]
  pot, force, total, _ = ir.rows(x, sp, q)
  return pot, force, total, ir.k_max(x, sp, q), ir.tau(x, sp, q)


def _call(dev, x, q, sp, want_pot=True, want_force=True, fill=None, stream=None, out=None):
  """cnf_interaction through the C ABI on device tensors x [S, N, D], q [S, Q, D] or None: (sums [S], pot [S, rows] or
  None, force [S, rows, D] or None).  out: a former result to write into (nothing is allocated, nothing waited for)."""
  from cnf_ot_amd import _capi, utils
  from cnf_ot_amd.flows import _stream_ptr
  spec = utils.interaction_spec(**ir.kwargs(sp))
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


def _composed(x, q, sp):
  """The torch float32 composition on the device, direct differences, the pair matrices reduced in float64, rows
  chunked: (pot [rows], force [rows, D], sum) as float64 numpy, pot and force as means over n"""
  a = x if q is None else q
  n = len(x) - 1 if q is None else len(x)
  pots, forces = [], []
  for i0 in range(0, len(a), 1024):
    diff = a[i0:i0 + 1024, None, :] - x[None, :, :]
    d2 = (diff * diff).sum(-1)
    if sp["kind"] == "quadratic":
      W, w = np.float32(0.5 * sp["amp"][0]) * d2, torch.full_like(d2, sp["amp"][0])
    else:
      W, w = torch.zeros_like(d2), torch.zeros_like(d2)
      r = torch.sqrt(d2)
      inv = torch.where(r > 0, 1.0 / r, torch.zeros_like(r))
      for amp, bw in zip(sp["amp"], sp["bw"]):
        if sp["kind"] == "gaussian":
          e = np.float32(amp) * torch.exp(-d2 / np.float32(2.0 * bw * bw))
          w = w - e / np.float32(bw * bw)
        else:
          e = np.float32(amp) * torch.exp(-r / np.float32(bw))
          w = w - e / np.float32(bw) * inv
        W = W + e
    if q is None:
      k = torch.arange(len(W), device=W.device)
      W[k, i0 + k] = 0.0
      w[k, i0 + k] = 0.0
    pots.append(W.double().sum(1))
    forces.append((diff * w[:, :, None]).double().sum(1))
  pot, force = torch.cat(pots), torch.cat(forces)
  return (pot / n).cpu().numpy(), (force / n).cpu().numpy(), float(pot.sum())


def _check(dev, x, q, sp, ref, tag, got=None):
  """One set against the restatement `ref` = (pot, force, sum, k_max, tau) under the bounds above; got: its (sums
  scalar, pot [rows], force [rows, D]) from a call made elsewhere (default: calls of its own, which also show that sums
  does not depend on what else is asked for)."""
  xd = torch.from_numpy(x).to(dev)
  qd = None if q is None else torch.from_numpy(q).to(dev)
  if got is None:
    q1 = None if qd is None else qd[None]
    sums, pot, force, _ = _call(dev, xd[None], q1, sp)
    for wp, wf in ((False, False), (True, False), (False, True)):
      s2, p2, f2, _ = _call(dev, xd[None], q1, sp, want_pot=wp, want_force=wf)
      assert torch.equal(sums, s2) and (p2 is None or torch.equal(p2, pot)) and (f2 is None or torch.equal(f2, force))
    got = (sums[0], pot[0], force[0])
  ref_pot, ref_force, ref_sum, k_max, tau = ref
  rows, n = len(ref_pot), (len(x) - 1 if q is None else len(x))
  comp_pot, comp_force, comp_sum = _composed(xd, qd, sp)
  got_pot, got_force = got[1].cpu().double().numpy(), got[2].cpu().double().numpy()
  norm = float(rows) * n
  e = {"sum": (abs(float(got[0]) - ref_sum) / norm, abs(comp_sum - ref_sum) / norm, 4.0 * EPS * k_max),
       "pot": (float(np.abs(got_pot - ref_pot).max()), float(np.abs(comp_pot - ref_pot).max()), 4.0 * EPS * k_max),
       "force": (float(np.abs(got_force - ref_force).max()), float(np.abs(comp_force - ref_force).max()), 4.0 * EPS * tau)}
  print(f"\n[interaction {tag}] mean {ref_sum / norm:.6f} | " + " | ".join(
    f"{k}: fused {a:.2e} composed {b:.2e} floor {c:.2e}" for k, (a, b, c) in e.items()))
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
  _check(dev, x, q, _specs(D)[name], _reference(D, Q, N, index, name), f"{name} D={D} Q={Q} N={N}")


def test_the_boundaries_named_above_are_the_kernels(dev):
  from cnf_ot_amd import _capi
  lib = _capi.lib()
  assert lib.cnf_interaction_splits(1, 64, 0, 2) == 1 and lib.cnf_interaction_splits(1, 65, 0, 2) == 2
  assert lib.cnf_interaction_splits(1, 63, 511, 2) == 1 and lib.cnf_interaction_splits(1, 65, 513, 2) == 2
  assert lib.cnf_interaction_splits(1, 512, 0, 2) == 8 and lib.cnf_interaction_splits(1, 513, 0, 2) == 9
  assert lib.cnf_interaction_splits(1, 5000, 0, 2) == 40       # two tiles of 64 columns per split
  src = open(os.path.join(os.path.dirname(_capi.__file__), "csrc", "cnf_interaction.hip")).read()
  assert "IA_THREADS = 256;" in src and "IA_R = 2;" in src and "IA_TILE = 64;" in src


@pytest.mark.parametrize("name", SPEC_NAMES)
def test_three_sets_with_their_own_data(dev, name):
  D, N, Q, S = 2, 257, 130, 3
  x, q = _inputs(D, Q, N, 40, S=S)
  x[1] *= np.float32(1.25)                               # (the sets differ in law as well as in draw)
  sp = _specs(D)[name]
  xd, qd = torch.from_numpy(x).to(dev), torch.from_numpy(q).to(dev)
  for mode, qq in (("self", None), ("query", qd)):
    sums, pot, force, _ = _call(dev, xd, qq, sp)
    for s in range(S):
      qs = None if qq is None else q[s]
      pr, fr, total, _ = ir.rows(x[s], sp, qs)
      _check(dev, x[s], qs, sp, (pr, fr, total, ir.k_max(x[s], sp, qs), ir.tau(x[s], sp, qs)), f"S=3 set {s} {mode} {name}",
             got=(sums[s], pot[s], force[s]))
    vals = [float(v) for v in sums]
    assert len({round(v / (N * N), 5) for v in vals}) == S           # three different numbers: no set read twice


@pytest.mark.parametrize("name", ["gaussian/4", "morse", "quadratic"])
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
    # views at an offset that is 4-byte but not 16-byte aligned
    bx = torch.zeros(x.size + 1, dtype=torch.float32, device=dev)
    xv = bx[1:].view(S, N, D).copy_(xd)
    qv = None
    if qq is not None:
      bq = torch.zeros(q.size + 3, dtype=torch.float32, device=dev)
      qv = bq[3:].view(S, Q, D).copy_(qd)
      assert qv.data_ptr() % 16 == 12
    assert xv.data_ptr() % 16 == 4
    assert same(base, _call(dev, xv, qv, sp))
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


@pytest.mark.parametrize("name", SPEC_NAMES)
def test_query_mode_on_the_particles_holds_the_diagonal(dev, name):
  D, N = 2, 600
  x, _ = _inputs(D, 0, N, 43)
  sp = _specs(D)[name]
  xd = torch.from_numpy(x).to(dev)[None]
  s_self, p_self, _, _ = _call(dev, xd, None, sp)
  s_q, p_q, f_q, _ = _call(dev, xd, xd.clone(), sp)
  diag = 0.0 if name == "quadratic" else sum(sp["amp"])      # W(0) per row
  floor = 4.0 * EPS * ir.k_max(x, sp)
  e_sum = abs(float(s_q[0] - s_self[0]) - N * diag) / (float(N) * N)
  e_pot = float((p_q[0].double() * N - p_self[0].double() * (N - 1) - diag).abs().max()) / N
  print(f"[interaction diagonal {name}] sums {e_sum:.2e} pot {e_pot:.2e} floor {floor:.2e}")
  assert e_sum <= floor and e_pot <= floor and torch.isfinite(f_q).all()


def test_coincident_points_with_the_exponential_kind(dev):
  D, N = 3, 150
  x, _ = _inputs(D, 0, N, 44)
  x[100:120] = x[:20]                                     # duplicated rows
  sp = _specs(D)["morse"]
  pr, fr, total, _ = ir.rows(x, sp)
  _, force = _check(dev, x, None, sp, (pr, fr, total, ir.k_max(x, sp), ir.tau(x, sp)), "morse, coincident points")
  assert np.isfinite(force).all()
  assert np.array_equal(force[100:120], force[:20])       # equal points, equal forces: the 0 of a coincident pair


def test_the_quadratic_identity_on_the_device(dev):
  from cnf_ot_amd import utils
  D, N, amp = 2, 600, 0.75
  x, _ = _inputs(D, 0, N, 45)
  sp = ir.spec("quadratic", [amp])
  res = utils.interaction_energy(x, "quadratic", [amp], want_grad=True, want_field=True)
  x64 = x.astype(np.float64)
  c = x64 - x64.mean(0)
  want_F = 0.5 * amp * np.trace(np.cov(x64.T))
  e_F = abs(float(res["energy"][0]) - want_F)
  e_f = float(np.abs(res["grad"].cpu().double().numpy() * N - amp * N / (N - 1.0) * c).max())
  f_F, f_f = 2.0 * EPS * ir.k_max(x, sp), 4.0 * EPS * ir.tau(x, sp)
  print(f"[interaction quadratic identity] F {want_F:.6f}: {e_F:.2e} (floor {f_F:.2e}) | force {e_f:.2e} (floor {f_f:.2e})")
  assert e_F <= f_F and e_f <= f_f


def test_far_clusters_underflow_to_exactly_zero(dev):
  D, N = 3, 300
  x, _ = _inputs(D, 0, N, 42)
  x[150:] += np.float32(1000.0)
  sp = ir.spec("gaussian", [1.0], _f32([0.1]))
  xd = torch.from_numpy(x).to(dev)
  sums, pot, force, _ = _call(dev, xd[None], None, sp)
  assert torch.isfinite(sums).all() and torch.isfinite(pot).all() and torch.isfinite(force).all()
  # the cross-cluster pairs: one cluster as the query points of the other
  cross, cpot, cforce, _ = _call(dev, xd[None, 150:].contiguous(), xd[None, :150].contiguous(), sp)
  assert ir.sums(x[150:], sp, x[:150]) == 0.0
  assert float(cross[0]) == 0.0 and not cpot.any() and not cforce.any()
  assert abs(float(sums[0]) - ir.sums(x, sp)) <= 4.0 * EPS * N * (N - 1)


@pytest.mark.parametrize("name", ["gaussian/4", "morse", "quadratic"])
def test_the_python_surface(dev, name):
  from cnf_ot_amd import utils
  D, N, Q = 2, 257, 130
  x, q = _inputs(D, Q, N, 46)
  sp = _specs(D)[name]
  kw = ir.kwargs(sp)
  a = utils.interaction_energy(x, want_grad=True, want_field=True, **kw)
  b = utils.interaction_energy(torch.from_numpy(x).to(dev).double()[None], **kw)
  assert set(a) == {"energy", "sums", "potential", "grad"} and set(b) == {"energy", "sums"}
  assert a["energy"].shape == (1,) and a["energy"].dtype == torch.float64 and a["sums"].shape == (1,)
  assert a["potential"].shape == (N,) and a["grad"].shape == (N, D) and a["grad"].dtype == torch.float32
  assert torch.equal(a["energy"], b["energy"])
  xd, qd = torch.from_numpy(x).to(dev)[None], torch.from_numpy(q).to(dev)[None]
  sums, pot, force, _ = _call(dev, xd, None, sp)
  assert torch.equal(a["sums"], sums) and torch.equal(a["potential"], pot[0]) and torch.equal(a["grad"], force[0] * (1.0 / N))
  assert float(a["energy"][0]) == float(sums[0]) / (2.0 * N * (N - 1.0))
  assert abs(float(a["energy"][0]) - ir.energy(x, sp)) <= 2.0 * EPS * ir.k_max(x, sp)
  f = utils.interaction_field(q, x, **kw)
  g = utils.interaction_field(q, x, want_force=False, **kw)
  sq, pq, fq, _ = _call(dev, xd, qd, sp)
  assert set(f) == {"potential", "force", "sums"} and set(g) == {"potential", "sums"}
  assert f["potential"].shape == (Q,) and f["force"].shape == (Q, D)
  assert torch.equal(f["sums"], sq) and torch.equal(f["potential"], pq[0]) and torch.equal(f["force"], fq[0])
  assert torch.equal(g["potential"], pq[0])


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("name", ["gaussian/4", "morse", "quadratic"])
def test_training_term_against_the_float64_adjoint(dev, D, name):
  import sample_term_check
  from cnf_ot_amd import applications as app, autograd
  B = 96
  sp = _specs(D)[name]
  kw = ir.kwargs(sp)
  none = np.zeros((1, D), dtype=np.float32)      # (the shared harness hands every term a target: this one has none)
  sample_term_check.check(
      dev, f"interaction_loss_fn D={D} {name}", D, B, none,
      lambda model, dim, params, tgt, cond, rng, batch, **k: app.interaction_loss_fn(model, dim, params, cond, rng, batch, **k),
      kw, auto=lambda x, y: autograd.interaction_energy(x, **kw),
      restate=lambda out: (ir.energy(out, sp), ir.xgrad(out, sp), None),
      floor=lambda out64, runs: 2.0 * EPS * max(ir.k_max(o, sp) for o in out64))


def test_one_time_autograd_against_the_fast_path(dev):
  from cnf_ot_amd import FlowConfig, FlowModel, Params, applications as app, autograd
  D, B = 2, 96
  cfg = FlowConfig(dim=D)
  params = Params.random(cfg, 0.2, seed=9, device=dev)
  model = FlowModel(cfg)
  kw = ir.kwargs(_specs(D)["morse"])
  g = torch.zeros_like(params.flat)
  loss = app.interaction_loss_fn(model, D, params, [0.5], 5, B, grad=g, **kw)
  be = model.terms_backend(params)
  flat_t = params.flat.clone().requires_grad_(True)
  samples, _ = autograd.flow_forward(be, flat_t, be.normal(5, B), torch.tensor([0.5], device=dev))
  val = autograd.interaction_energy(samples, **kw)
  val.sum().backward()
  assert val.shape == (1,) and float(val.detach()[0]) == float(loss)
  e = float((flat_t.grad - g).abs().max())
  print(f"[interaction_loss_fn, one time] autograd against the fast path: {e:.2e} (|g| {float(g.abs().max()):.2e})")
  assert e <= B * 2.0 ** -24 * float(g.abs().max())


def _composite(which, model, dim, params, rng, batch, tbs, **kw):
  from cnf_ot_amd import applications as app
  if which == "rwpo":
    return app.rwpo_loss_fn(model, dim, 2, 10, 0.01, 0.01, tbs, "double_well", 1, params, rng, 5000.0, batch, **kw)
  return app.ot_loss_fn(model, dim, 1, 0.01, tbs, which, params, rng, 5000.0, batch, **kw)


@pytest.mark.parametrize("which", ["free", "obstacle", "rwpo"])
@pytest.mark.parametrize("name", ["morse", "quadratic"])
def test_composites_gain_the_interaction_part(dev, which, name):
  from cnf_ot_amd import FlowConfig, FlowModel, Params, applications as app
  from cnf_ot_amd.distributed import Shard
  dim, batch, tbs, rng, strength = 2, 2048, 4, 11, 0.7
  T = 2 if which == "rwpo" else 1
  sub = batch // 32
  cfg = FlowConfig(dim=dim)
  params = Params.random(cfg, 0.2, seed=6, device=dev)
  model = FlowModel(cfg)
  kw = ir.kwargs(_specs(dim)[name])
  g0, g1, gi = (torch.zeros_like(params.flat) for _ in range(3))
  base = _composite(which, model, dim, params, rng, batch, tbs, grad=g0)
  full = _composite(which, model, dim, params, rng, batch, tbs, grad=g1, interaction=(kw, strength))
  # (the loss without a gradient is its own route through the loss kernels: it gains the same part)
  base_plain = _composite(which, model, dim, params, rng, batch, tbs)
  plain = _composite(which, model, dim, params, rng, batch, tbs, interaction=(kw, strength))
  times = app.draw_t_batch(rng, tbs, float(T))
  part = app.interaction_loss_fn(model, dim, params, times, rng, sub, grad=gi, **kw)
  torch.cuda.synchronize()
  assert full.dtype == torch.float64 and part.dtype == torch.float64
  # the value: one addition in float64 (the precision `combine` returns), of the product strength T part
  want = float(base) + strength * T * float(part)
  e_v = abs(float(full) - want)
  assert abs(float(plain) - (float(base_plain) + strength * T * float(part))) <= 2.0 ** -52 * abs(want)
  # the gradient, (terms accumulated) 2^-24 max |g| in two parts: the part's pass accumulates tbs * sub sample adjoints in
  # float32 (scaled by strength T before the pass here, after it in `want_g`) at the part's own scale, and the loss's
  # three or four terms and the part are added into one float32 tensor at the scale of the whole gradient
  terms = (3 if which == "free" else 4) + 1
  want_g = g0.double() + strength * T * gi.double()
  e_g = float((g1.double() - want_g).abs().max())
  bound = 2.0 ** -24 * (tbs * sub * strength * T * float(gi.abs().max()) + terms * float(want_g.abs().max()))
  print(f"[{which} + {name}] loss {float(base):.6f} + {strength * T * float(part):.6f}: error {e_v:.2e} | gradient "
        f"|.| {float(want_g.abs().max()):.3e}: error {e_g:.2e} (bound {bound:.2e})")
  assert e_v <= 2.0 ** -52 * abs(want)
  assert e_g <= bound
  # the part's samples are the first `sub` rows of the loss's own draw: its values are the stand-alone call's, bit for bit
  ctx = app._Ctx(model, params, rng, Shard(0, 1))
  ctx.noise(batch)
  inside = app._interaction_values(ctx, app.ia.interaction_spec(**kw), times, sub, strength * T)
  assert float(inside.sum() / tbs) == float(part)


def test_it_trains(dev):
  from cnf_ot_amd import applications as app, solvers, utils
  dim, B, rng = 2, 512, 3
  config = solvers.load_config(overrides={"general": {"dim": dim}})
  model = solvers.build_model(config)
  params = model.init(0)
  loss_fn = lambda p, r, _lambda, batch, grad=None: app.interaction_loss_fn(model, dim, p, [0.5], r, batch, "quadratic", [1.0],
                                                                            grad=grad)
  trace = lambda: float(utils.point_stats(model.apply.sample(params, cond=0.5, seed=rng, sample_shape=(B,)))["cov"][0].trace())
  opt = solvers.Adam(1e-3)
  state = opt.init(params)
  update = solvers.make_update(loss_fn, opt, B)
  before, tr_before = float(loss_fn(params, rng, 0.0, B)), trace()
  for _ in range(60):
    _, params, state = update(params, rng, 0.0, state)
  after, tr_after = float(loss_fn(params, rng, 0.0, B)), trace()
  print(f"[interaction, 60 Adam steps, quadratic] loss {before:.6f} -> {after:.6f} | tr cov at t = 0.5 {tr_before:.6f} -> "
        f"{tr_after:.6f}")
  assert after < before and tr_after < tr_before


@pytest.mark.parametrize("_type,kind", [("ot", "quadratic"), ("rwpo", "exponential")])
def test_evaluate_interaction_equals_its_composition(dev, _type, kind):
  from cnf_ot_amd import FlowConfig, Params, solvers, utils
  dim, n, seed = 2, 2048, 5
  ia = {"kind": kind, "strength": 2.0, "amplitudes": [0.75] if kind == "quadratic" else [1.0, -0.5], "bandwidths": [0.5, 2.0]}
  config = solvers.load_config(overrides={"general": {"type": _type, "dim": dim}, "interaction": ia})
  model = solvers.build_model(config)
  params = Params.random(FlowConfig(dim=dim), 0.2, seed=4, device=dev)
  res = solvers.evaluate_interaction(config, model, params, n=n, seed=seed)
  assert set(res) == set(solvers.INTERACTION_KEYS)
  T = 1.0 if _type == "ot" else 2.0
  ts = np.linspace(0.0, T, 9)
  assert res["times"] == [float(t) for t in ts] and res["n"] == n // 2 and res["kind"] == kind and res["strength"] == 2.0
  draws = [model.apply.sample(params, cond=float(t), seed=seed, sample_shape=(n,)) for t in ts]
  kw = {"kind": kind, "amplitudes": ia["amplitudes"], "bandwidths": None if kind == "quadratic" else ia["bandwidths"]}
  both = utils.interaction_energy(torch.stack([d[:n // 2] for d in draws] + [d[n // 2:] for d in draws]), **kw)["energy"]
  first, second = both[:9], both[9:]      # (one call over the 18 sets, as the evaluation makes it: the split count is S's)
  assert np.array_equal(np.array(res["energy"]), first.cpu().numpy())
  assert np.array_equal(np.array(res["floor"]), (first - second).abs().cpu().numpy())
  F = first.cpu().numpy()
  assert abs(res["running_cost"] - 2.0 * float(((F[1:] + F[:-1]) * 0.5 * np.diff(ts)).sum())) <= 1e-12 * abs(res["running_cost"])
  if kind == "quadratic":
    sp = ir.spec("quadratic", ia["amplitudes"])
    for s, d in enumerate(draws):
      floor = 2.0 * EPS * ir.k_max(d[:n // 2].cpu().numpy(), sp)
      print(f"[evaluate_interaction t={ts[s]:.3f}] energy {res['energy'][s]:.6f} trace_cov {res['trace_cov'][s]:.6f} "
            f"difference {abs(res['energy'][s] - res['trace_cov'][s]):.2e} (floor {floor:.2e}) MC floor {res['floor'][s]:.2e}")
      assert abs(res["energy"][s] - res["trace_cov"][s]) <= floor
  else:
    assert res["trace_cov"] is None
  solvers.print_interaction(res)
