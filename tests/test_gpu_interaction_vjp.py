"""The interacting Fokker-Planck training term on the GPU: cnf_interaction_vjp / utils.interaction_force_vjp /
autograd.interaction_force / cnf_score_residual_force / applications.fp_loss_fn(interaction=...) /
solvers.evaluate_mv_path, against the float64 restatements (tests/interaction_vjp_ref.py, flow_adjoint_f64.py).

The pair pass is held to test_gpu_interaction.py's bar with its EPS = 5e-6 (derived there: a float32 accumulator lives
for one tile of 64 columns, 64 * 2^-24 = 3.8e-6 of the tile's largest term times its length, and the per-term roundings
stay below 5e-7 of that term's bound):
  e_fused <= 2 e_composed + floor,   floor = 4 EPS eta max_{k,j} |g_k - g_j|   (errors in the max-norm of xbar),
because xbar_k is a MEAN over N - 1 pairs of H(x_k - x_j) (g_k - g_j), each of which is at most eta |g_k - g_j| in the
Euclidean norm, eta the largest operator norm of the pair Hessian: sum_b |amp_b| / bw_b^2 for the Gaussian kind
(|c1| <= that, and |c1 + c2 d^2| = |sum_b amp_b / bw_b^2 (d^2 / bw_b^2 - 1) e_b| <= it as well, since |s - 1| e^(-s/2)
<= 1); read from the restatement over the cloud's own pairs for the exponential kind (w / r grows without bound as two
points approach) and the quadratic kind (|amp_0|).  The per-term roundings are the force's plus the difference g_k - g_j,
the dot product's fmaf chain and two fmafs per coordinate: still below 5e-7 eta |g_k - g_j| each.  e_composed is the
torch float32 composition of the same sum (direct differences, the pair tensors reduced in float64).

The kernel's boundaries, each with a shape below, at and above it: IA_TILE = 64 columns (N = 63, 64, 65; the column split
exceeds 1 from N = 65), IA_ROWS = 512 rows per workgroup (511, 512, 513), a second row group with splits (1025).

The epilogue with a force is held to test_gpu_step_kernels.py's bounds for cnf_score_residual at its shapes, with the
force's term in T_d = |r2 - r1| / dt + |coef score_d| + M_d + |strength force_d| and ONE more rounding (the fmaf that adds
strength force_d): 12 EPS' where that test has 11, 20 where it has 19 (EPS' = 2^-24), and |d fbar| <= 12 EPS' 2 c
|strength| T_d.

Measured on one MI355X (every test prints its figures: run with -s):
  pair pass, largest e_fused / (2 e_composed + floor) per spec over the ten shapes, the three sets and the duplicated
    rows: gaussian/1 0.0023, gaussian/2 0.0006, gaussian/3 0.0006, gaussian/4 0.0004, morse 0.0031, quadratic 0.0067
    (fused errors 1.5e-8 .. 3.9e-7 against floors of 7e-5 .. 2.5e-2; the composition is at the same level)
  epilogue with force, worst error / bound over the 63 cases: rbar12 0.51, rbar3 0.43, sbar 0.44, fbar 0.43
  fp_loss_fn(interaction=...): the seven calls by hand bit for bit; against the float64 restatement (rows kept, gradient
    error / bound): D=2 gradient 63 rows 2.2e-2 / 3.7e-1 (Gaussian x 2), 2.3e-2 / 4.8e-1 (Morse); D=3 lorenz 62 rows
    5.6e-3 / 6.6e-2, 5.8e-3 / 7.6e-2; D=10 ou 46 rows 8.8e-4 / 2.3e-3, 8.8e-4 / 2.1e-3.  On the WHOLE draw at D=10 the
    gradient missed (5.3e-3 against 3.4e-3), with the force's strength 0 as well (5.26e-3): one conditioner's block
    (mlp_layer1_d8) at 9 x its bound, 16 of the 192 score evaluations within the ReLU margin -- the flow's backward
    across a ReLU, which test_gpu_flow_adjoint.py removes from its inputs for the same reason
  100 Adam steps: loss 120.17 -> 11.26, tr cov at T 1.9918 -> 0.2400 (mean-field 0.3375, free 1.1353)
More: profiles/interaction_vjp/README.md.
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
import flow_adjoint_f64 as fa
import interaction_ref as ir
import interaction_vjp_ref as ivr
import step_kernels_ref as sk

EPS = 5e-6                                   # test_gpu_interaction.py's, derived there
SHAPES = [(1, 2), (2, 63), (2, 64), (2, 65), (2, 511), (2, 512), (2, 513), (3, 1025), (10, 300), (14, 129)]      # (D, N)


def _f32(v):
  return [float(np.float32(a)) for a in v]      # (as the kernel receives them)


def _specs(D):
  """test_gpu_interaction.py's four specs, and a Gaussian each with 2 and 3 terms"""
  r = math.sqrt(D)
  return {"gaussian/1": ir.spec("gaussian", [1.0], _f32([r])),
          "gaussian/4": ir.spec("gaussian", [1.0, -0.5, 0.25, -0.75], _f32([0.5 * r, r, 2.0 * r, 4.0 * r])),
          "morse": ir.spec("exponential", [1.0, -0.5], [0.5, 2.0]),
          "quadratic": ir.spec("quadratic", [0.75]),
          "gaussian/2": ir.spec("gaussian", [1.0, -0.5], _f32([0.5 * r, 2.0 * r])),
          "gaussian/3": ir.spec("gaussian", [-1.0, 0.5, 0.25], _f32([0.5 * r, r, 3.0 * r]))}


SPEC_NAMES = list(_specs(1))
SHARE = {}                                   # spec name -> the largest e_fused / (2 e_composed + floor) seen


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def _inputs(D, N, index, S=None):
  """(x, g) [N, D] -- [S, N, D] with S"""
  x = ir.cloud(D, N, 5000 + index, scale=1.0 + 0.125 * (index % 5), S=S)
  g = ir.cloud(D, N, 6000 + index, scale=0.75, S=S)
  return x, g


def _eta(x, sp):
  if sp["kind"] == "gaussian":
    return sum(abs(a) / (b * b) for a, b in zip(sp["amp"], sp["bw"]))
  return ivr.hessian_norm(x, sp)


@functools.lru_cache(maxsize=None)
def _reference(D, N, index, name):
  """The restatement of one (shape, spec) case, computed once: (xbar, floor)"""
  x, g = _inputs(D, N, index)
  sp = _specs(D)[name]
  return ivr.force_vjp(x, g, sp), 4.0 * EPS * _eta(x, sp) * ivr.pair_spread(g)


def _call(dev, x, g, sp, fill=None, stream=None, out=None):
  """cnf_interaction_vjp through the C ABI on device tensors x, g [S, N, D]: (xbar [S, N, D], workspace).  out: a former
  result to write into (nothing is allocated, nothing waited for)."""
  from cnf_ot_amd import _capi, utils
  from cnf_ot_amd.flows import _stream_ptr
  spec = utils.interaction_spec(**ir.kwargs(sp))
  S, N, D = x.shape
  lib = _capi.lib()
  nbytes = ctypes.c_int64(0)
  _capi.check(lib.cnf_interaction_vjp_workspace(S, N, D, ctypes.byref(nbytes)), "cnf_interaction_vjp_workspace")
  if out is None:
    ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
    if fill is not None:
      ws.fill_(fill)
    xbar = torch.full((S, N, D), 7.25, dtype=torch.float32, device=dev)
  else:
    xbar, ws = out
  assert x.is_contiguous() and g.is_contiguous() and x.dtype == g.dtype == torch.float32 and g.shape == x.shape
  _capi.check(lib.cnf_interaction_vjp(ctypes.byref(spec), S, x.data_ptr(), g.data_ptr(), N, D, xbar.data_ptr(), ws.data_ptr(),
                                      nbytes.value, _stream_ptr(dev) if stream is None else stream), "cnf_interaction_vjp")
  if out is None:
    torch.cuda.synchronize()
  return xbar, ws


def _composed(x, g, sp):
  """The torch float32 composition on the device: direct differences, the pair tensors reduced in float64, rows chunked"""
  N = len(x)
  outs = []
  for i0 in range(0, N, 1024):
    diff = x[i0:i0 + 1024, None, :] - x[None, :, :]
    dv = g[i0:i0 + 1024, None, :] - g[None, :, :]
    d2 = (diff * diff).sum(-1)
    if sp["kind"] == "quadratic":
      c1, c2 = torch.full_like(d2, sp["amp"][0]), torch.zeros_like(d2)
    else:
      c1, c2 = torch.zeros_like(d2), torch.zeros_like(d2)
      r = torch.sqrt(d2)
      inv = torch.where(r > 0, 1.0 / r, torch.zeros_like(r))
      for amp, bw in zip(sp["amp"], sp["bw"]):
        if sp["kind"] == "gaussian":
          e = np.float32(amp) * torch.exp(-d2 / np.float32(2.0 * bw * bw))
          c1 = c1 - e / np.float32(bw * bw)
          c2 = c2 + e / np.float32(bw ** 4)
        else:
          e = np.float32(amp) * torch.exp(-r / np.float32(bw))
          c1 = c1 - e / np.float32(bw) * inv
          c2 = c2 + (e / np.float32(bw * bw)) * inv * inv + (e / np.float32(bw)) * inv * inv * inv
    k = torch.arange(len(d2), device=d2.device)
    c1[k, i0 + k] = 0.0
    c2[k, i0 + k] = 0.0
    dot = (diff * dv).sum(-1)
    outs.append((c1[:, :, None] * dv + diff * (dot * c2)[:, :, None]).double().sum(1))
  return (torch.cat(outs) / (N - 1.0)).cpu().numpy()


def _check(dev, x, g, sp, name, ref, floor, tag, got=None):
  xd, gd = torch.from_numpy(x).to(dev), torch.from_numpy(g).to(dev)
  if got is None:
    got = _call(dev, xd[None], gd[None], sp)[0][0]
  got = got.cpu().double().numpy()
  comp = _composed(xd, gd, sp)
  e_f, e_c = float(np.abs(got - ref).max()), float(np.abs(comp - ref).max())
  share = e_f / (2.0 * e_c + floor)
  SHARE[name] = max(SHARE.get(name, 0.0), share)
  print(f"\n[interaction vjp {tag}] |xbar| {np.abs(ref).max():.3e}: fused {e_f:.2e} composed {e_c:.2e} floor {floor:.2e} "
        f"| fused / (2 composed + floor) {share:.4f} (largest so far for {name}: {SHARE[name]:.4f})")
  assert np.isfinite(got).all()
  assert e_f <= 2.0 * e_c + floor, (tag, e_f, e_c, floor)
  return got


@pytest.mark.parametrize("name", SPEC_NAMES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "D%d-N%d" % s)
def test_pair_pass_against_the_restatement(dev, shape, name):
  D, N = shape
  index = SHAPES.index(shape)
  x, g = _inputs(D, N, index)
  ref, floor = _reference(D, N, index, name)
  _check(dev, x, g, _specs(D)[name], name, ref, floor, f"{name} D={D} N={N}")


def test_the_boundaries_named_above_are_the_kernels(dev):
  from cnf_ot_amd import _capi
  lib = _capi.lib()
  assert lib.cnf_interaction_splits(1, 64, 0, 2) == 1 and lib.cnf_interaction_splits(1, 65, 0, 2) == 2
  assert lib.cnf_interaction_splits(1, 512, 0, 2) == 8 and lib.cnf_interaction_splits(1, 1025, 0, 3) == 17
  src = open(os.path.join(os.path.dirname(_capi.__file__), "csrc", "cnf_interaction_pairs.h")).read()
  assert "IA_THREADS = 256;" in src and "IA_R = 2;" in src and "IA_TILE = 64;" in src
  nbytes = ctypes.c_int64(0)
  assert lib.cnf_interaction_vjp_workspace(1, 1025, 3, ctypes.byref(nbytes)) == 0 and nbytes.value == 8 * 17 * 1025 * 3


@pytest.mark.parametrize("name", SPEC_NAMES)
def test_three_sets_with_their_own_data(dev, name):
  D, N, S = 2, 257, 3
  x, g = _inputs(D, N, 40, S=S)
  x[1] *= np.float32(1.25)                               # (the sets differ in law as well as in draw)
  sp = _specs(D)[name]
  xbar, _ = _call(dev, torch.from_numpy(x).to(dev), torch.from_numpy(g).to(dev), sp)
  for s in range(S):
    floor = 4.0 * EPS * _eta(x[s], sp) * ivr.pair_spread(g[s])
    _check(dev, x[s], g[s], sp, name, ivr.force_vjp(x[s], g[s], sp), floor, f"S=3 set {s} {name}", got=xbar[s])
  assert not torch.equal(xbar[0], xbar[1]) and not torch.equal(xbar[1], xbar[2])      # no set read twice


@pytest.mark.parametrize("name", ["gaussian/4", "morse", "quadratic"])
def test_a_row_duplicated_at_a_distant_index(dev, name):
  D, N = 3, 700
  x, g = _inputs(D, N, 44)
  x[600:620] = x[:20]                                     # (another workgroup's rows and another split's columns)
  sp = _specs(D)[name]
  floor = 4.0 * EPS * _eta(x, sp) * ivr.pair_spread(g)
  got = _check(dev, x, g, sp, name, ivr.force_vjp(x, g, sp), floor, f"{name}, duplicated rows")
  assert np.isfinite(got).all()
  # with equal adjoints too, the duplicates receive equal results: their own pair gives 0 either way
  g[600:620] = g[:20]
  again = _call(dev, torch.from_numpy(x).to(dev)[None], torch.from_numpy(g).to(dev)[None], sp)[0][0].cpu().numpy()
  assert np.array_equal(again[600:620], again[:20])


@pytest.mark.parametrize("name", ["gaussian/3", "morse", "quadratic"])
def test_reproducibility(dev, name):
  D, N, S = 3, 700, 2
  x, g = _inputs(D, N, 41, S=S)
  sp = _specs(D)[name]
  xd, gd = torch.from_numpy(x).to(dev), torch.from_numpy(g).to(dev)
  base = _call(dev, xd, gd, sp)[0]
  assert torch.equal(base, _call(dev, xd, gd, sp)[0])                          # two calls
  assert torch.equal(base, _call(dev, xd, gd, sp, fill=0xFF)[0])               # (0xFF bytes: NaN doubles wherever a word is read unwritten)
  # views at an offset that is 4-byte but not 16-byte aligned
  bx, bg = torch.zeros(x.size + 1, dtype=torch.float32, device=dev), torch.zeros(x.size + 3, dtype=torch.float32, device=dev)
  xv, gv = bx[1:].view(S, N, D).copy_(xd), bg[3:].view(S, N, D).copy_(gd)
  assert xv.data_ptr() % 16 == 4 and gv.data_ptr() % 16 == 12
  assert torch.equal(base, _call(dev, xv, gv, sp)[0])
  # one call replayed from a captured graph: a single stream, one linear chain of launches, nothing allocated
  replay = _call(dev, xd.flip(1).contiguous(), gd, sp)
  torch.cuda.synchronize()
  side = torch.cuda.Stream(device=dev)
  side.wait_stream(torch.cuda.current_stream(dev))
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side):
    _call(dev, xd, gd, sp, stream=side.cuda_stream, out=replay)
  replay[0].fill_(7)
  graph.replay()
  torch.cuda.synchronize()
  assert torch.equal(base, replay[0])


@pytest.mark.parametrize("name", ["gaussian/4", "morse", "quadratic"])
def test_the_python_surface_and_the_autograd_function(dev, name):
  from cnf_ot_amd import autograd, utils
  D, N = 2, 257
  x, g = _inputs(D, N, 46)
  sp = _specs(D)[name]
  kw = ir.kwargs(sp)
  xd, gd = torch.from_numpy(x).to(dev), torch.from_numpy(g).to(dev)
  raw = _call(dev, xd[None], gd[None], sp)[0]
  a = utils.interaction_force_vjp(x, g, **kw)                                  # host inputs, one set
  b = utils.interaction_force_vjp(xd.double()[None], gd[None], **kw)           # device, float64 x, [1, N, D]
  assert a.shape == (N, D) and a.dtype == torch.float32 and b.shape == (1, N, D)
  assert torch.equal(a, raw[0]) and torch.equal(b, raw)
  # more than 64 sets: one call per 64, set by set the single call's bits
  xs, gs = _inputs(D, 33, 47, S=66)
  many = utils.interaction_force_vjp(xs, gs, **kw)
  for s in (0, 63, 64, 65):
    assert torch.equal(many[s], utils.interaction_force_vjp(xs[s], gs[s], **kw))
  # autograd.interaction_force: forward = the force of utils.interaction_energy's call, backward = interaction_force_vjp
  xt = xd.clone().requires_grad_(True)
  f = autograd.interaction_force(xt, **kw)
  res = utils.interaction_energy(xd, want_grad=True, **kw)
  assert f.shape == (N, D) and f.dtype == torch.float32 and torch.equal(f.detach() * (1.0 / N), res["grad"])
  f.backward(gd)
  assert torch.equal(xt.grad, a)
  x3 = torch.from_numpy(xs[:3]).to(dev).requires_grad_(True)
  (autograd.interaction_force(x3, **kw) * torch.from_numpy(gs[:3]).to(dev)).sum().backward()
  assert torch.equal(x3.grad, many[:3])


def test_share_of_the_bound_per_spec(dev):
  """(runs after the cases above in file order: prints what they recorded)"""
  for name, share in SHARE.items():
    print(f"[interaction vjp] {name}: largest e_fused / (2 e_composed + floor) = {share:.4f}")
    assert share <= 1.0


# =====================================================================================================================
# cnf_score_residual_force
# =====================================================================================================================
EPS24 = 2.0 ** -24
SCORE_DRIFTS = [(1, None), (2, None), (2, "ou"), (2, "gradient"), (2, "nongradient"), (3, "lorenz"), (3, "ou"), (6, "ou"),
                (14, None)]
SCORE_SHAPES = [(1, 1), (1000, 1), (1000, 63), (4096, 64), (4099, 65), (777, 1000), (65537, 4096)]
DT, COEF, DRIFT_A, LOSS_COEF, STRENGTH = 0.01, 0.7, 1.3, 0.37, 1.7


def _drift_magnitudes(drift, r3, a):
  """test_gpu_step_kernels.py's: the sums of the absolute monomials of drift_d and of d drift_d / d r_e"""
  n, D = r3.shape
  M, MJ = np.zeros((n, D)), np.zeros((n, D, D))
  if drift == "ou":
    M = a * np.abs(r3)
    MJ[:, np.arange(D), np.arange(D)] = a
  elif drift == "gradient":
    x, y = np.abs(r3[:, 0]), np.abs(r3[:, 1])
    q = x * x + y * y + 4.0
    M[:, 0], M[:, 1] = a * q * x, a * (q * y + 2 * y + 2)
    MJ[:, 0, 0], MJ[:, 1, 1] = a * (q + 2 * x * x), a * (q + 2 * y * y + 2)
    MJ[:, 0, 1] = MJ[:, 1, 0] = a * 2 * x * y
  elif drift == "nongradient":
    x, y = np.abs(r3[:, 0]), np.abs(r3[:, 1])
    M[:, 0], M[:, 1] = a * x + 0.5 * y, a * y + 0.5 * x
    MJ[:, 0, 0] = MJ[:, 1, 1] = a
    MJ[:, 0, 1] = MJ[:, 1, 0] = 0.5
  elif drift == "lorenz":
    x, y, z = np.abs(r3[:, 0]), np.abs(r3[:, 1]), np.abs(r3[:, 2])
    M[:, 0], M[:, 1], M[:, 2] = 10 * (x + y), 28 * x + 9 * x * z + y, 9 * x * y + 8 * z / 3
    MJ[:, 0, 0] = MJ[:, 0, 1] = 10.0
    MJ[:, 1, 0], MJ[:, 1, 1], MJ[:, 1, 2] = 28 + 9 * z, 1.0, 9 * x
    MJ[:, 2, 0], MJ[:, 2, 1], MJ[:, 2, 2] = 9 * y, 9 * x, 8.0 / 3.0
  return M, MJ


def _force_call(dev, r, score, force, strength, n, count, D, drift, adjoints):
  from cnf_ot_amd import _capi
  sums = torch.full((-(-n // count),), 7.25, dtype=torch.float64, device=dev)
  rbar, sbar, fbar = (torch.full(s, 7.25, dtype=torch.float32, device=dev) for s in ((3 * n, D), (n, D), (n, D)))
  ptr = lambda t: t.data_ptr() if adjoints else None
  rc = _capi.lib().cnf_score_residual_force(r.data_ptr(), score.data_ptr(), force.data_ptr(), strength, n, count, D, DT, COEF,
                                            sk.DRIFT_CODES[drift], DRIFT_A, LOSS_COEF, sums.data_ptr(), ptr(rbar), ptr(sbar),
                                            ptr(fbar), None)
  torch.cuda.synchronize()
  assert rc == _capi.CNF_OK, rc
  if not adjoints:
    assert all(bool((t == 7.25).all()) for t in (rbar, sbar, fbar))
  return sums.cpu().numpy(), rbar, sbar, fbar


@pytest.mark.parametrize("n,count", SCORE_SHAPES)
@pytest.mark.parametrize("D,drift", SCORE_DRIFTS)
def test_epilogue_with_force_sums_and_adjoints(dev, D, drift, n, count):
  from cnf_ot_amd import _capi
  f32 = lambda v: float(np.float32(v))
  rng = np.random.default_rng(1000 * D + n + count)
  r = (1.5 * rng.normal(size=(3 * n, D))).astype(np.float32)
  score = rng.normal(size=(n, D)).astype(np.float32)
  force = rng.normal(size=(n, D)).astype(np.float32)
  dt, coef, a, c, kappa = f32(DT), f32(COEF), f32(DRIFT_A), f32(LOSS_COEF), f32(STRENGTH)
  want_sums, want_rbar, want_sbar, want_fbar = ivr.score_residual_force_ref(r, score, force, kappa, n, count, D, dt, coef, drift,
                                                                           a, c)
  rd, sd, fd = (torch.from_numpy(v).to(dev) for v in (r, score, force))
  sums0, _, _, _ = _force_call(dev, rd, sd, fd, STRENGTH, n, count, D, drift, adjoints=False)
  sums1, rbar, sbar, fbar = _force_call(dev, rd, sd, fd, STRENGTH, n, count, D, drift, adjoints=True)
  atol = 2e-6 * np.abs(want_sums).max() / min(count, 100)
  for name, sums in (("value", sums0), ("value+adjoints", sums1)):
    err = np.abs(sums - want_sums)
    print(f"[score_residual_force D={D} {drift} n={n} count={count} {name}] sums worst err / (atol + rtol |want|) "
          f"{(err / (atol + 2e-6 * np.abs(want_sums))).max():.3f}")
    assert (err <= atol + 2e-6 * np.abs(want_sums)).all()
  r64 = r.astype(np.float64)
  M, MJ = _drift_magnitudes(drift, r64[2 * n:], a)
  T = np.abs(r64[n:2 * n] - r64[:n]) / dt + np.abs(coef * score.astype(np.float64)) + M + np.abs(kappa * force.astype(np.float64))
  b12 = 12 * EPS24 * (2 * c / dt) * T
  b3 = np.zeros_like(T) if drift is None else 12 * EPS24 * 2 * c * a * T if drift == "ou" else \
      20 * EPS24 * 2 * c * np.einsum("id,ide->ie", T, MJ)
  bound_r = np.concatenate([b12, b12, b3])
  bound_s, bound_f = 12 * EPS24 * 2 * c * coef * T, 12 * EPS24 * 2 * c * kappa * T
  got_r, got_s, got_f = (t.cpu().numpy() for t in (rbar, sbar, fbar))
  er, es, ef = np.abs(got_r - want_rbar), np.abs(got_s - want_sbar), np.abs(got_f - want_fbar)
  worst3 = (er[2 * n:] / b3).max() if drift is not None else 0.0
  print(f"[score_residual_force D={D} {drift} n={n} count={count}] worst err / bound: rbar12 {(er[:2 * n] / bound_r[:2 * n]).max():.3f} "
        f"rbar3 {worst3:.3f} sbar {(es / bound_s).max():.3f} fbar {(ef / bound_f).max():.3f}")
  assert np.isfinite(got_r).all() and np.isfinite(got_s).all() and np.isfinite(got_f).all()
  assert (er <= bound_r).all() and (es <= bound_s).all() and (ef <= bound_f).all()
  if drift is None:
    assert not got_r[2 * n:].any()
  # strength 0 is cnf_score_residual on the same inputs: fma(0, force, u) is u, so the adjoints carry its bits (the sums
  # meet in double atomics whose order is free: to the rule above) and fbar is 0
  sums_z, rbar_z, sbar_z, fbar_z = _force_call(dev, rd, sd, fd, 0.0, n, count, D, drift, adjoints=True)
  rbar_p, sbar_p, sums_p = torch.empty_like(rbar), torch.empty_like(sbar), torch.empty(-(-n // count), dtype=torch.float64, device=dev)
  rc = _capi.lib().cnf_score_residual(rd.data_ptr(), sd.data_ptr(), n, count, D, DT, COEF, sk.DRIFT_CODES[drift], DRIFT_A,
                                      LOSS_COEF, sums_p.data_ptr(), rbar_p.data_ptr(), sbar_p.data_ptr(), None)
  torch.cuda.synchronize()
  assert rc == _capi.CNF_OK
  assert torch.equal(rbar_z, rbar_p) and torch.equal(sbar_z, sbar_p) and not fbar_z.any()
  want_plain = sk.score_residual_ref(r, score, n, count, D, dt, coef, drift, a, c)[0]
  atol_p = 2e-6 * np.abs(want_plain).max() / min(count, 100)
  assert (np.abs(sums_z - want_plain) <= atol_p + 2e-6 * np.abs(want_plain)).all()
  assert (np.abs(sums_p.cpu().numpy() - want_plain) <= atol_p + 2e-6 * np.abs(want_plain)).all()


# =====================================================================================================================
# applications.fp_loss_fn(interaction=...)
# =====================================================================================================================
FP_CASES = [(2, "gradient"), (3, "lorenz"), (10, "ou")]
FP_SPECS = {"gaussian/2": lambda D: ir.spec("gaussian", [1.0, -0.5], _f32([0.5 * math.sqrt(D), 2.0 * math.sqrt(D)])),
            "morse": lambda D: ir.spec("exponential", [1.0, -0.5], [0.5, 2.0])}
BATCH, TBS, RNG, T_FP, A_FP, SIGMA, KAPPA = 2048, 3, 21, 1.0, 1.0, 0.5, 0.8


def _fp(app, model, D, sub, params, _lambda, **kw):
  return app.fp_loss_fn(model, D, T_FP, A_FP, SIGMA, 0.01, 0.01, TBS, sub, params, RNG, _lambda, BATCH, **kw)


def _by_hand(app, model, D, sub, params, _lambda, spec, strength, grad, rows=None):
  """fp_loss_fn(interaction=...) as its seven calls, issued here; rows: on those rows of the flow-matching term's draw
  alone (the coefficients stay the full draw's)"""
  from cnf_ot_amd import _capi, interaction as ia
  from cnf_ot_amd.distributed import Shard
  ctx = app._Ctx(model, params, RNG, Shard(0, 1), grad)
  be = ctx.be
  t_batch = app.draw_t_batch(RNG, TBS, T_FP)
  sub_n = BATCH // 32
  c_rkl, c_fm = _lambda / BATCH, 0.5 * T_FP / (sub_n * TBS)
  rkl = app._reverse_kl_sum(ctx, T_FP, 4.0, 0.0, BATCH, c_rkl)
  z, _, count = ctx.noise(sub_n)
  if rows is not None:
    z, count = z[torch.as_tensor(rows, device=z.device)].contiguous(), len(rows)
  th = app._conds(t_batch)
  S = len(th)
  n = S * count
  half = np.float32(0.005)
  tt = be.slice_conds(th)
  conds3 = app._cat_conds([th - half, th + half, th])
  z3 = z.repeat(3 * S, 1)
  r, _ = be.forward_logdet(z3, be.slice_conds(conds3), want_logdet=False)                          # 1
  r3 = r[2 * n:]
  sets = r3.view(S, count, -1)
  force = ia._call(spec, sets, None, False, True)[2].view(n, -1)                                 # 2
  score = be.logprob_fd(r3, tt, 0.01)                                                            # 3
  sums, rbar, sbar, fbar = be.score_residual_force(r, score, force, strength, count, 0.01, SIGMA, _capi.DRIFTS[sub], A_FP,
                                                   c_fm, True)                                   # 4
  rbar[2 * n:] += ia._vjp_call(spec, sets, fbar.view(S, count, -1)).view(n, -1)                  # 5
  rbar[2 * n:] += be.logprob_fd_vjp(r3, tt, 0.01, sbar, grad)                                    # 6
  ctx.defer_pass_vjp(z3, conds3, count, rbar, None)                                              # 7 (leaves in combine)
  return ctx.combine([rkl, sums], [c_rkl, c_fm])


def _term_f64(cfg, flat, z, th, count, sub, sp, strength, c_fm, dtype):
  """The flow-matching term with the force, c_fm sum |u|^2, and its parameter gradient, from flow_adjoint_f64's passes
  in `dtype` with the pair sums, the epilogue and the drift in float64 (interaction_vjp_ref)"""
  net = fa._Net(cfg, flat, dtype)
  S, D = len(th), z.shape[1]
  n = S * count
  half = np.float32(0.005)
  f = lambda v: np.asarray(v, dtype=dtype)
  c3 = np.repeat(np.concatenate([th - half, th + half, th]).astype(np.float32), count)
  z3 = f(np.tile(z, (3 * S, 1)))
  r, _, recs, _, _ = fa._forward(net, z3, f(c3), False)
  r3 = r[2 * n:]
  score, evals, _, _ = fa._fd_score(net, r3, f(np.repeat(th.astype(np.float32), count)), f(np.float32(0.01)))
  r64 = r.astype(np.float64)
  sets = r64[2 * n:].reshape(S, count, D)
  force = np.concatenate([ir.force(sets[s], sp) for s in range(S)])
  dt, coef, a = (float(np.float32(v)) for v in (0.01, SIGMA, A_FP))
  kappa, c = float(np.float32(strength)), float(np.float32(c_fm))
  sums, rbar, sbar, fbar = ivr.score_residual_force_ref(r64, score.astype(np.float64), force, kappa, n, count, D, dt, coef,
                                                        sub, a, c)
  fb = fbar.reshape(S, count, D)
  rbar[2 * n:] += np.concatenate([ivr.force_vjp(sets[s], fb[s], sp) for s in range(S)])
  r3b, grad = fa._fd_score_bwd(net, evals, f(sbar), f(np.float32(0.01)))
  rbar = f(rbar)
  rbar[2 * n:] += r3b
  grad = grad + fa._backward(net, recs, rbar, None, False, 3 * n)[1]
  return c_fm * float(sums.sum()), np.asarray(grad, dtype=np.float64)


def _kept_rows(cfg, flat, z, th):
  """The rows of the draw z whose 3 S pass points and 2 D S evaluation points all keep flow_adjoint_f64's margins from
  every knot and ReLU in the float64 pass (a float32 evaluation can land on the other side of those, where the
  parameter gradient jumps): chosen from the reference alone, before anything is compared"""
  S, B = len(th), len(z)
  half = np.float32(0.005)
  c3 = np.repeat(np.concatenate([th - half, th + half, th]).astype(np.float32), B)
  z3 = np.tile(z, (3 * S, 1))
  knot, relu = fa.margins(cfg, flat, z3, c3, False)
  r3 = fa.pass_vjp(cfg, flat, z3, c3, None, None, False)[0][2 * S * B:]
  fk, fr = fa.fd_margins(cfg, flat, r3, np.repeat(th.astype(np.float32), B), float(np.float32(0.01)))
  knot = np.minimum(knot.reshape(3 * S, B).min(0), fk.reshape(S, B).min(0))
  relu = np.minimum(relu.reshape(3 * S, B).min(0), fr.reshape(S, B).min(0))
  return np.nonzero((knot >= fa.KNOT_MARGIN) & (relu >= fa.RELU_MARGIN))[0]


@pytest.mark.parametrize("name", list(FP_SPECS))
@pytest.mark.parametrize("D,sub", FP_CASES)
def test_fp_loss_with_the_interaction(dev, D, sub, name):
  """Value and gradient against the seven calls issued by hand (bit for bit: the same launches in the same order),
  against the float64 restatement on the rows that keep flow_adjoint_f64's margins (gradient: flow_adjoint_f64.bound with
  its knot term, as test_gpu_flow_adjoint.py holds the difference terms; value: twice the float32 restatement's own error
  plus the knots' and 1e-6 of the value), and interaction=None against the entry points it ran before."""
  from cnf_ot_amd import FlowConfig, FlowModel, Params, applications as app, interaction as ia
  from cnf_ot_amd.distributed import Shard
  cfg = FlowConfig(dim=D)
  params = Params.random(cfg, float(fa._scale(D)), seed=6 + D, device=dev)
  model = FlowModel(cfg)
  sp = FP_SPECS[name](D)
  kw = ir.kwargs(sp)
  spec = ia.interaction_spec(**kw)
  for _lambda in (5000.0, 0.0):
    g1, g2 = torch.zeros_like(params.flat), torch.zeros_like(params.flat)
    full = _fp(app, model, D, sub, params, _lambda, grad=g1, interaction=(kw, KAPPA))
    hand = _by_hand(app, model, D, sub, params, _lambda, spec, KAPPA, g2)
    plain = _fp(app, model, D, sub, params, _lambda, interaction=(kw, KAPPA))
    torch.cuda.synchronize()
    assert full.dtype == torch.float64 and float(full) == float(hand) and torch.equal(g1, g2)
    if _lambda == 0.0:      # (with a weight, the reverse-KL term without a gradient is another kernel's sum)
      assert abs(float(plain) - float(full)) <= 1e-12 * abs(float(full))     # (the sums' double atomics: order is free)
  # the float64 restatement of the flow-matching term (_lambda = 0: the reverse-KL term has coefficient 0), on the rows of
  # the loss's own draw that keep the margins -- through the seven calls, which ARE fp_loss_fn bit for bit (above).  At
  # dim 10 a sample has 3 + 20 evaluations through 18 conditioners each: on the whole draw one ReLU that the kernels and
  # the float64 pass take on different sides put mlp_layer1_d8 at 9 x its bound, with the force's strength 0 as well
  be = model.terms_backend(params)
  sub_n = BATCH // 32
  z_all = be.normal(RNG, BATCH)[:sub_n].cpu().numpy()
  th = np.asarray(app._conds(app.draw_t_batch(RNG, TBS, T_FP)), dtype=np.float32)
  flat = params.flat.cpu().numpy()
  c_fm = 0.5 * T_FP / (sub_n * TBS)
  rows = _kept_rows(cfg, flat, z_all, th)
  assert len(rows) >= sub_n // 2, len(rows)
  z = z_all[rows]
  gs = torch.zeros_like(params.flat)
  got = _by_hand(app, model, D, sub, params, 0.0, spec, KAPPA, gs, rows=rows)
  torch.cuda.synchronize()
  ref = lambda dt: _term_f64(cfg, flat, z, th, len(rows), sub, sp, KAPPA, c_fm, dt)
  (v64, g64), (v32, g32) = ref(np.float64), ref(np.float32)
  # (the knots' rounding to float32, which one float32 run shows only by luck: 1 / dt = 100 amplifies it in the
  # difference (r2 - r1) / dt, test_gpu_flow_adjoint.py's reason for the same term)
  k_v, k_g = fa.knot_sensitivity(lambda: ref(np.float64), (v64, g64))
  e_v, e_g = abs(float(got) - v64), float(np.abs(gs.cpu().double().numpy() - g64).max())
  bound = fa.bound(g32, g64, knots=k_g)
  print(f"\n[fp_loss_fn + {name} D={D} {sub}] {len(rows)} of {sub_n} rows | loss {v64:.6f}: error {e_v:.2e} (float32 restatement "
        f"{abs(v32 - v64):.2e}, knots {float(k_v):.2e}) | gradient |.| {np.abs(g64).max():.3e}: error {e_g:.2e}, bound {bound:.2e} "
        f"(without the knots' term {fa.bound(g32, g64):.2e})")
  assert e_v <= 2.0 * abs(v32 - v64) + float(k_v) + 1e-6 * abs(v64)
  assert e_g <= bound
  # the force matters: the same loss without it is another number
  g0, gh = torch.zeros_like(params.flat), torch.zeros_like(params.flat)
  none = _fp(app, model, D, sub, params, 5000.0, grad=g0, interaction=None)
  ctx = app._Ctx(model, params, RNG, Shard(0, 1), gh)
  t_batch = app.draw_t_batch(RNG, TBS, T_FP)
  c_rkl = 5000.0 / BATCH
  c_fm = 0.5 * T_FP / (sub_n * TBS)
  want = ctx.combine([app._reverse_kl_sum(ctx, T_FP, 4.0, 0.0, BATCH, c_rkl),
                      app._flow_matching_sum(ctx, D, A_FP, SIGMA, sub, t_batch, sub_n, c_fm)], [c_rkl, c_fm])
  torch.cuda.synchronize()
  assert float(none) == float(want) and torch.equal(g0, gh)
  assert float(none) != float(_fp(app, model, D, sub, params, 5000.0, interaction=(kw, KAPPA)))


# =====================================================================================================================
# training on the interacting problem, and the evaluation beside the particle reference
# =====================================================================================================================
TRAIN_STEPS = 100


def _train_config():
  from cnf_ot_amd import solvers
  return solvers.load_config(overrides={
    "general": {"type": "fp", "dim": 2, "t_batch_size": 4, "seed": 7},
    "fp": {"T": 1, "a": 1, "sigma": 0.5, "velocity_field_type": "ou"},
    "train": {"epochs": TRAIN_STEPS, "lr": 0.005, "_lambda": 5000.0, "batch_size": 2048, "eval_frequency": 100},
    "interaction": {"kind": "quadratic", "strength": 2.0, "amplitudes": [1.0], "role": "drift"}})


@pytest.fixture(scope="module")
def trained(dev):
  """(config, model, trained parameters, loss history, tr cov at T before and after)"""
  from cnf_ot_amd import solvers, utils
  config = _train_config()
  model = solvers.build_model(config)
  tr = lambda p: float(utils.point_stats(model.apply.sample(p, cond=1.0, seed=3, sample_shape=(8192,)))["cov"][0].trace())
  before = tr(model.init(config["general"]["seed"]))           # (the identity flow train() starts from)
  model, params, hist = solvers.train(config)
  return config, model, params, [float(h) for h in hist], before, tr(params)


def test_it_trains_towards_the_mean_field_limit(dev, trained):
  """fp / ou at dim 2, a = 1, sigma = 0.5, T = 1 with the quadratic kernel (amp 1) at strength 2 in the drift: the
  mean-field variance per dimension at T is mv_quadratic_ou_variance = 0.169 (tr cov 0.338), the free OU value 0.568
  (tr cov 1.136).  Measured: 100 Adam steps (lr 5e-3, 0.03 s) take the loss (mean of 10 steps) from 120.17 to 11.26 and tr
  cov at T from 1.9918 to 0.2400; 50 steps reach 0.4382, 150 0.2348, 300 0.2428 (profiles/interaction_vjp/README.md)."""
  from cnf_ot_amd import applications as app
  config, model, params, hist, before, after = trained
  mf = 2 * app.mv_quadratic_ou_variance(1.0, 1.0, 0.5, 2.0, 1.0, app.fp_initial_variance(1))
  free = 2 * app.ou_variance(1.0, 1.0, app.fp_initial_variance(1), 0.5)
  first, last = float(np.mean(hist[:10])), float(np.mean(hist[-10:]))
  print(f"\n[interacting fp, {TRAIN_STEPS} Adam steps] loss {first:.4f} -> {last:.4f} | tr cov at T {before:.4f} -> {after:.4f} "
        f"(mean-field {mf:.4f}, free {free:.4f})")
  assert abs(mf - 0.338) < 2e-3 and abs(free - 1.136) < 2e-3
  assert last < first
  assert abs(after - mf) < abs(after - free)
  assert not abs(before - mf) < abs(before - free)


def test_evaluate_mv_path_beside_the_reference(dev, trained):
  from cnf_ot_amd import solvers
  config, model, params = trained[:3]
  args = dict(times=[0.0, 0.5, 1.0], n_particles=256, replicas=2, h=1e-2, seed=5)
  res = solvers.evaluate_mv_path(config, model, params, n=512, **args)
  ref = solvers.evaluate_mv_reference(config, **args)
  assert set(res) == set(solvers.MV_PATH_KEYS)
  for k in ("times", "mean", "trace_cov", "trace_cov_floor", "energy", "energy_floor", "free_trace_cov", "trace_cov_exact", "bad",
            "kind", "strength", "replicas"):
    assert res[k] == ref[k], k
  assert res["n"] == 512 and res["n_particles"] == 256 and res["trace_cov_exact"] is not None
  for k in ("flow_mean", "flow_trace_cov", "flow_energy"):
    assert len(res[k]) == 3 and np.isfinite(np.array(res[k])).all(), k
  # the quadratic kind: F = amp tr(cov) / 2 with the unbiased covariance
  for F, trc in zip(res["flow_energy"], res["flow_trace_cov"]):
    assert abs(F - 0.5 * trc * 512 / 511.0) <= 1e-4 * abs(F)
  solvers.print_mv_path(res)
