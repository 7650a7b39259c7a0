"""The fused kernel two-sample statistics on the GPU: cnf_mmd2 / utils.mmd2 / autograd.mmd2 / applications.mmd_loss_fn /
solvers.evaluate_fp_two_sample, against the float64 restatement (tests/mmd_ref.py), with the torch float32 composition
of the same estimator -- direct differences, pair matrices reduced in float64 -- as the yardstick for the fused error:
  e_fused <= 2 e_composed + floor,   floor = 4 eps k_max (value),  4 eps tau (N xgrad, max-norm over rows),
eps = 5e-6 per mean: a 64-term float32 partial sum errs by at most 64 * 2^-24 = 3.8e-6 relative, per-term rounding stays
below 5e-7 k_max (max a e^-a = 0.37 bounds the effect of the argument's rounding), and the estimator combines its means
with weights 1, 1, 2.  Gaussian: k_max = n_bw, tau = sum_b 0.61 / bw_b; energy: k_max = the largest pair distance of the
restatement, tau = 1.

The kernel's own boundaries, each with a shape below, at and above it (BOUNDARY_SHAPES): 512 rows per workgroup (N = 511,
512, 513), 64 columns per tile (M = 63, 64, 65), and the column split, which exceeds 1 from the first shape whose longer
side leaves one tile: max(N, M) = 65, i.e. N M = 65 * 2 (the split count is cnf_mmd_splits, asserted below).

Measured on one MI355X (every test prints its figures: run with -s), errors against the restatement, fused / composed:
  the 56 (shape, kernel) cases   value up to 6.5e-7 / 3.3e-7 (floors 2e-5 .. 2.1e-4: at most 0.004 of the floor),
                                 N xgrad up to 6.9e-7 / 1.9e-7 (floors 6.5e-6 .. 4.9e-5: at most 0.03 of the floor)
  D=2 N=257 M=130 Gaussian x 3   value 8.8e-10 / 1.9e-9    N xgrad 2.5e-7 / 3.0e-8
  D=2 N=5000 M=3000 energy       value 6.0e-11 / 2.5e-10   N xgrad 1.2e-7 / 6.6e-9
  D=14 N=129 M=64 energy         value 3.0e-7 / 1.0e-9     N xgrad 5.1e-7 / 1.9e-8
  mmd_loss_fn, D = 2 / 3         loss 3.0e-8 / 7.6e-9 (Gaussian), 8.9e-8 / 6.2e-8 (energy); parameter gradient 1.2e-7 / 1.1e-7
                                 and 2.5e-7 / 1.9e-7 against flow_adjoint_f64.bound = 3.5e-6 / 1.9e-6 and 8.6e-6 / 4.5e-6;
                                 autograd.mmd2(flow_forward(...)) gave the fast path's gradient bit for bit
  evaluate_fp_two_sample, ou     mmd2 0.64 .. 1.01 beside floors of 3e-5 .. 2.4e-3 in size (random parameters)
More cases: profiles/mmd/README.md.
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
import mmd_ref as mr

EPS = 5e-6
ISSUE_SHAPES = [(1, 2, 2), (1, 65, 63), (2, 257, 130), (3, 64, 64), (2, 256, 512), (10, 300, 257), (14, 129, 64),
                (2, 5000, 3000)]
# (D, N, M): rows per workgroup 512 and columns per tile 64, below / at / above; the split count 1 -> 2 at max(N, M) 64 -> 65
BOUNDARY_SHAPES = [(2, 511, 63), (2, 512, 64), (2, 513, 65), (3, 64, 2), (3, 65, 2), (2, 1025, 1024)]
KERNELS = [("gaussian", 1), ("gaussian", 3), ("gaussian", 8), ("energy", 0)]


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def _bws(D, n_bw):
  return [math.sqrt(D) * 0.5 * 2.0 ** b for b in range(n_bw)]


def _spec(kind, D, n_bw):
  # the bandwidths as the kernel receives them (float32)
  return mr.spec(kind, [float(np.float32(b)) for b in _bws(D, n_bw)] if kind == "gaussian" else ())


def _inputs(D, N, M, index, S=None):
  return mr.clouds(D, N, M, seed=1000 + index, shift=0.2 + 0.1 * (index % 4), scale=1.0 + 0.125 * (index % 5), S=S)


def _call(dev, x, y, sp, want_grad=True, fill=None):
  """cnf_mmd2 through the C ABI on device tensors x [S, N, D], y [S, M, D]: (sums [S, 3], xgrad [S, N, D] or None)"""
  from cnf_ot_amd import _capi, utils
  from cnf_ot_amd.flows import _stream_ptr
  spec, _ = utils.mmd_spec(sp["bw"], sp["kind"])
  S, N, D = x.shape
  M = y.shape[1]
  lib = _capi.lib()
  nbytes = ctypes.c_int64(0)
  _capi.check(lib.cnf_mmd_workspace(S, N, M, D, int(want_grad), ctypes.byref(nbytes)), "cnf_mmd_workspace")
  ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
  if fill is not None:
    ws.fill_(fill)
  sums = torch.empty(S, 3, dtype=torch.float64, device=dev)
  grad = torch.empty(S, N, D, dtype=torch.float32, device=dev) if want_grad else None
  assert x.is_contiguous() and y.is_contiguous() and x.dtype == torch.float32 and y.dtype == torch.float32
  _capi.check(lib.cnf_mmd2(ctypes.byref(spec), S, x.data_ptr(), N, y.data_ptr(), M, D, sums.data_ptr(),
                           None if grad is None else grad.data_ptr(), ws.data_ptr(), nbytes.value, _stream_ptr(dev)),
              "cnf_mmd2")
  torch.cuda.synchronize()
  return sums, grad


def _composed(x, y, sp):
  """The torch float32 composition on the device, direct differences, the pair matrices reduced in float64:
  (mmd2, N xgrad [N, D]) as float64 numpy"""
  N, M = len(x), len(y)

  def block(a, b, skip):
    diff = a[:, None, :] - b[None, :, :]
    d2 = (diff * diff).sum(-1)
    if sp["kind"] == "energy":
      d = torch.sqrt(d2)
      k, w = -d, torch.where(d > 0, 1.0 / d, torch.zeros_like(d))
    else:
      k, w = torch.zeros_like(d2), torch.zeros_like(d2)
      for bw in sp["bw"]:
        e = torch.exp(-d2 / np.float32(2.0 * bw * bw))
        k = k + e
        w = w + e / np.float32(bw * bw)
    if skip:
      k.fill_diagonal_(0.0)
      w.fill_diagonal_(0.0)
    return k.double().sum(), -(diff * w[:, :, None]).double().sum(1)

  (sxx, gxx), (syy, _), (sxy, gxy) = block(x, x, True), block(y, y, True), block(x, y, False)
  val = sxx / (N * (N - 1.0)) + syy / (M * (M - 1.0)) - 2.0 * sxy / (float(N) * M)
  g = 2.0 / (N - 1.0) * gxx - 2.0 / M * gxy
  return float(val), g.cpu().numpy()


def _check(dev, x, y, sp, tag, got=None):
  """One set against the restatement under the bounds above; got: its (sums [3], xgrad [N, D]) from a call made
  elsewhere (default: a call of its own).  Returns (N xgrad of the fused call, N xgrad of the restatement)."""
  N, M = len(x), len(y)
  xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
  if got is None:
    sums, grad = _call(dev, xd[None], yd[None], sp)
    sums_only, _ = _call(dev, xd[None], yd[None], sp, want_grad=False)
    assert torch.equal(sums, sums_only)                    # the value does not depend on whether the gradient is asked for
    got = (sums[0], grad[0])
  ref_val, ref_g = mr.mmd2(x, y, sp), mr.xgrad(x, y, sp) * N
  got_val = mr.mmd2_of_sums(got[0].cpu().numpy(), N, M)
  got_g = got[1].cpu().double().numpy() * N
  comp_val, comp_g = _composed(xd, yd, sp)
  e_val, e_comp = abs(got_val - ref_val), abs(comp_val - ref_val)
  e_g, e_gcomp = float(np.abs(got_g - ref_g).max()), float(np.abs(comp_g - ref_g).max())
  f_val, f_g = 4.0 * EPS * mr.k_max(x, y, sp), 4.0 * EPS * mr.tau(sp)
  print(f"\n[mmd {tag}] value {ref_val:.6f}: fused {e_val:.2e} composed {e_comp:.2e} floor {f_val:.2e} | "
        f"N xgrad (|.| {np.abs(ref_g).max():.3f}): fused {e_g:.2e} composed {e_gcomp:.2e} floor {f_g:.2e}")
  assert np.isfinite(got_val) and np.isfinite(got_g).all()
  assert e_val <= 2.0 * e_comp + f_val, (tag, e_val, e_comp, f_val)
  assert e_g <= 2.0 * e_gcomp + f_g, (tag, e_g, e_gcomp, f_g)
  return got_g, ref_g


@pytest.mark.parametrize("kind,n_bw", KERNELS)
@pytest.mark.parametrize("shape", ISSUE_SHAPES + BOUNDARY_SHAPES, ids=lambda s: "D%d-N%d-M%d" % s)
def test_value_and_gradient_against_the_restatement(dev, shape, kind, n_bw):
  D, N, M = shape
  index = (ISSUE_SHAPES + BOUNDARY_SHAPES).index(shape)
  x, y = _inputs(D, N, M, index)
  _check(dev, x, y, _spec(kind, D, n_bw), f"{kind}/{n_bw} D={D} N={N} M={M}")


def test_the_boundaries_named_above_are_the_kernels(dev):
  from cnf_ot_amd import _capi
  lib = _capi.lib()
  assert lib.cnf_mmd_splits(1, 64, 2, 3) == 1 and lib.cnf_mmd_splits(1, 65, 2, 3) == 2
  assert lib.cnf_mmd_splits(1, 512, 64, 2) == 8 and lib.cnf_mmd_splits(1, 513, 65, 2) == 9
  assert lib.cnf_mmd_splits(1, 5000, 3000, 2) == 40        # two tiles of 64 columns per split
  src = open(os.path.join(os.path.dirname(_capi.__file__), "csrc", "cnf_mmd.hip")).read()
  assert "MMD_THREADS = 256;" in src and "MMD_R = 2;" in src and "MMD_TILE = 64;" in src


@pytest.mark.parametrize("kind,n_bw", [("gaussian", 3), ("energy", 0)])
def test_three_sets_with_their_own_data(dev, kind, n_bw):
  D, N, M, S = 2, 257, 130, 3
  x, y = _inputs(D, N, M, 40, S=S)
  y[1] += 0.25                                           # (the sets differ in law as well as in draw)
  sp = _spec(kind, D, n_bw)
  sums, grad = _call(dev, torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), sp)
  for s in range(S):
    _check(dev, x[s], y[s], sp, f"S=3 set {s} {kind}/{n_bw}", got=(sums[s], grad[s]))
  vals = [mr.mmd2_of_sums(sums[s].cpu().numpy(), N, M) for s in range(S)]
  assert len({round(v, 5) for v in vals}) == S           # three different numbers: no set read twice


@pytest.mark.parametrize("kind,n_bw", [("gaussian", 5), ("energy", 0)])
def test_reproducibility(dev, kind, n_bw):
  D, N, M, S = 3, 700, 1100, 2
  x, y = _inputs(D, N, M, 41, S=S)
  sp = _spec(kind, D, n_bw)
  xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
  s0, g0 = _call(dev, xd, yd, sp)
  s1, g1 = _call(dev, xd, yd, sp)
  assert torch.equal(s0, s1) and torch.equal(g0, g1)
  s2, g2 = _call(dev, xd, yd, sp, fill=0xFF)            # (0xFF bytes: NaN doubles wherever the workspace is not rewritten)
  assert torch.equal(s0, s2) and torch.equal(g0, g2)
  # views at an offset that is 4-byte but not 16-byte aligned
  bx = torch.zeros(x.size + 1, dtype=torch.float32, device=dev)
  by = torch.zeros(y.size + 3, dtype=torch.float32, device=dev)
  xv, yv = bx[1:].view(S, N, D), by[3:].view(S, M, D)
  xv.copy_(xd)
  yv.copy_(yd)
  assert xv.data_ptr() % 16 == 4 and yv.data_ptr() % 16 == 12
  s3, g3 = _call(dev, xv, yv, sp)
  assert torch.equal(s0, s3) and torch.equal(g0, g3)


def test_far_clouds_underflow_to_exactly_zero(dev):
  D, N, M = 3, 300, 200
  x, y = _inputs(D, N, M, 42)
  y = (y + np.float32(1000.0)).astype(np.float32)
  sp = mr.spec("gaussian", [float(np.float32(0.1))])
  sums, grad = _call(dev, torch.from_numpy(x).to(dev)[None], torch.from_numpy(y).to(dev)[None], sp)
  assert float(sums[0, 2]) == 0.0 and torch.isfinite(sums).all() and torch.isfinite(grad).all()
  ref = mr.sums(x, y, sp)
  assert ref[2] == 0.0 and abs(float(sums[0, 0]) - ref[0]) <= 4.0 * EPS * N * (N - 1)


@pytest.mark.parametrize("kind,n_bw", [("gaussian", 1), ("gaussian", 8), ("energy", 0)])
def test_a_cloud_against_itself(dev, kind, n_bw):
  D, N = 2, 600
  x, _ = _inputs(D, N, 2, 43)
  sp = _spec(kind, D, n_bw)
  xd = torch.from_numpy(x).to(dev)[None]
  sums, grad = _call(dev, xd, xd.clone(), sp)
  sxx, syy, sxy = (float(v) for v in sums[0])
  assert sxx == syy                                     # bit for bit: the same code on the same numbers
  # the xy block holds the diagonal the xx block leaves out: k(x, x) = n_bw per row (0 for the energy kernel)
  print(f"[mmd self {kind}/{n_bw}] sxy - sxx - N n_bw = {sxy - sxx - N * n_bw:.3e}")
  assert abs((sxy - sxx) / (float(N) * N) - n_bw / float(N)) <= 4.0 * EPS * mr.k_max(x, x, sp)
  assert torch.isfinite(grad).all()


def test_coincident_points_with_the_energy_kernel(dev):
  D, N, M = 3, 150, 90
  x, y = _inputs(D, N, M, 44)
  x[100:120] = x[:20]                                     # duplicated rows in x
  y[10:40] = x[30:60]                                     # rows of x repeated in y
  sp = mr.spec("energy")
  g, ref = _check(dev, x, y, sp, "energy, coincident points")
  assert np.isfinite(g).all()
  assert np.array_equal(g[100:120], g[:20])               # equal points, equal gradients: the 0 of a coincident pair
  # the restatement's own coincident pairs contribute 0: leaving the duplicates' partners out changes nothing else
  assert np.array_equal(ref[100:120], ref[:20])


@pytest.mark.parametrize("kind,n_bw", [("gaussian", 3), ("energy", 0)])
def test_symmetry_and_the_python_surface(dev, kind, n_bw):
  from cnf_ot_amd import utils
  D, N, M = 2, 257, 130
  x, y = _inputs(D, N, M, 45)
  sp = _spec(kind, D, n_bw)
  bws = sp["bw"] if kind == "gaussian" else None
  a = utils.mmd2(x, y, bws, kind, want_grad=True)
  b = utils.mmd2(torch.from_numpy(y).to(dev).double(), torch.from_numpy(x).to(dev), bws, kind)
  assert set(a) == {"mmd2", "sums", "bandwidths", "grad"} and set(b) == {"mmd2", "sums", "bandwidths"}
  assert a["mmd2"].shape == (1,) and a["mmd2"].dtype == torch.float64 and a["sums"].shape == (1, 3)
  assert a["grad"].shape == (N, D) and a["grad"].dtype == torch.float32 and a["bandwidths"] == (bws or [])
  floor = 4.0 * EPS * mr.k_max(x, y, sp)
  print(f"[mmd symmetry {kind}] mmd2(x, y) - mmd2(y, x) = {float(a['mmd2'][0] - b['mmd2'][0]):.3e} (floor {floor:.2e})")
  assert abs(float(a["mmd2"][0] - b["mmd2"][0])) <= floor
  assert abs(float(a["mmd2"][0]) - mr.mmd2(x, y, sp)) <= floor
  sums, grad = _call(dev, torch.from_numpy(x).to(dev)[None], torch.from_numpy(y).to(dev)[None], sp)
  assert torch.equal(a["sums"], sums) and torch.equal(a["grad"], grad[0])
  if kind == "gaussian":                                   # the default bandwidths: the median heuristic on y
    c = utils.mmd2(x, y)
    yy = y.astype(np.float64)
    d = np.sqrt(((yy[:, None] - yy[None]) ** 2).sum(-1))[np.triu_indices(M, 1)]
    med = np.sort(d)[(d.size - 1) // 2]
    assert np.allclose(c["bandwidths"], [f * med for f in (0.25, 0.5, 1.0, 2.0, 4.0)], rtol=1e-6)
    assert c["bandwidths"] == [float(np.float32(b)) for b in utils.median_bandwidths(torch.from_numpy(y))]


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("kind", ["gaussian", "energy"])
def test_training_term_against_the_float64_adjoint(dev, D, kind):
  import sample_term_check
  from cnf_ot_amd import applications as app, autograd
  B, M = 96, 130
  _, tgt = _inputs(D, 2, M, 46 + D)
  sp = _spec(kind, D, 3)
  bws = sp["bw"] if kind == "gaussian" else None
  samples = sample_term_check.check(
      dev, f"mmd_loss_fn D={D} {kind}", D, B, tgt, app.mmd_loss_fn, dict(bandwidths=bws, kind=kind),
      auto=lambda x, y: autograd.mmd2(x, y, bws, kind),
      restate=lambda out: (mr.mmd2(out, tgt, sp), mr.xgrad(out, tgt, sp), None),
      floor=lambda out64, runs: 4.0 * EPS * max(mr.k_max(o, tgt, sp) for o in out64))
  # ... and differentiable in y, by the call with the roles swapped
  yt = torch.from_numpy(tgt).to(dev).requires_grad_(True)
  xs = samples[:B]
  autograd.mmd2(xs, yt, bws, kind).sum().backward()
  e_y = float(np.abs(yt.grad.cpu().double().numpy() - mr.xgrad(tgt, xs.cpu().numpy(), sp)).max()) * M
  assert e_y <= 4.0 * EPS * mr.tau(sp) + 2e-6 * float(np.abs(mr.xgrad(tgt, xs.cpu().numpy(), sp)).max()) * M


def test_one_time_autograd_against_the_fast_path(dev):
  from cnf_ot_amd import FlowConfig, FlowModel, Params, applications as app, autograd
  D, B = 2, 96
  cfg = FlowConfig(dim=D)
  params = Params.random(cfg, 0.2, seed=9, device=dev)
  model = FlowModel(cfg)
  _, tgt = _inputs(D, 2, 130, 50)
  bws = _bws(D, 3)
  g = torch.zeros_like(params.flat)
  loss = app.mmd_loss_fn(model, D, params, tgt, [0.5], 5, B, bandwidths=bws, grad=g)
  be = model.terms_backend(params)
  flat_t = params.flat.clone().requires_grad_(True)
  samples, _ = autograd.flow_forward(be, flat_t, be.normal(5, B), torch.tensor([0.5], device=dev))
  val = autograd.mmd2(samples, torch.from_numpy(tgt).to(dev), bws)
  val.sum().backward()
  # the same cnf_mmd2 call on the same samples: the value bit for bit; the backward pass receives a zero log-det
  # adjoint where the fast path passes none: the gradient to float32 rounding of its accumulation
  assert float(val.detach()[0]) == float(loss)
  e = float((flat_t.grad - g).abs().max())
  print(f"[mmd_loss_fn, one time] autograd against the fast path: {e:.2e} (|g| {float(g.abs().max()):.2e})")
  assert e <= B * 2.0 ** -24 * float(g.abs().max())


@pytest.mark.parametrize("sub,dim", [("ou", 2), ("lorenz", 3)])
def test_evaluate_fp_two_sample_equals_its_composition(dev, sub, dim):
  from cnf_ot_amd import FlowConfig, Params, applications as app, solvers, utils
  from cnf_ot_amd.distributed import Shard
  config = solvers.load_config(overrides={"general": {"type": "fp", "dim": dim}, "fp": {"velocity_field_type": sub}})
  f = config["fp"]
  model = solvers.build_model(config)
  params = Params.random(FlowConfig(dim=dim), 0.2, seed=4, device=dev)
  n, h, seed = 4096, 1e-2, 5
  res = solvers.evaluate_fp_two_sample(config, model, params, n_particles=n, h=h, seed=seed)
  assert set(res) == {"times", "mmd2", "mmd2_floor", "energy", "energy_floor", "bandwidths"}
  ts = np.rint(solvers.figure_settings(config)["t_array"] / h) * h
  assert res["times"] == [float(t) for t in ts]
  h0, h1 = (app.fp_reference_particles(dim, f["T"], f["a"], f["sigma"], sub, ts, n, h, seed, positions=True,
                                       shard=Shard(r, 2), all_reduce=False)["pos"].float() for r in (0, 1))
  flow = torch.stack([model.apply.sample(params, cond=float(t), seed=seed, sample_shape=(n // 2,)) for t in ts])
  bws = utils.median_bandwidths(h0)
  assert res["bandwidths"] == [float(np.float32(b)) for b in bws] and len(bws) == 5
  want = {"mmd2": utils.mmd2(flow, h0, bws)["mmd2"], "mmd2_floor": utils.mmd2(h1, h0, bws)["mmd2"],
          "energy": utils.mmd2(flow, h0, kind="energy")["mmd2"], "energy_floor": utils.mmd2(h1, h0, kind="energy")["mmd2"]}
  for k, v in want.items():
    print(f"[evaluate_fp_two_sample {sub}] {k}: " + " ".join(f"{a:.3e}" for a in res[k]))
    assert np.array_equal(np.array(res[k]), v.cpu().numpy(), equal_nan=True), k
  assert np.isfinite(res["mmd2"][0]) and np.isfinite(res["energy"][0]) and res["mmd2"][0] > res["mmd2_floor"][0]
  solvers.print_fp_two_sample(res)
  # a user's bandwidths are used as given
  own = solvers.evaluate_fp_two_sample(config, model, params, times=[0.0, 0.1], n_particles=n, h=h, seed=seed, bandwidths=[0.7, 2.0])
  assert own["bandwidths"] == [float(np.float32(0.7)), 2.0] and len(own["mmd2"]) == 2


def test_an_identity_flow_stands_out_of_the_floor(dev):
  from cnf_ot_amd import FlowConfig, Params, solvers
  # T = 3: the ensemble starts from N(0, (T + 1) / 2 I) = N(0, 2 I); the identity flow samples N(0, I)
  config = solvers.load_config(overrides={"general": {"type": "fp", "dim": 2}, "fp": {"velocity_field_type": "ou", "T": 3.0}})
  model = solvers.build_model(config)
  res = solvers.evaluate_fp_two_sample(config, model, Params.zeros(FlowConfig(dim=2), dev), times=[0.0, 0.1], n_particles=4096,
                                       h=1e-2, seed=5)
  print(f"[identity flow against N(0, 2 I)] mmd2 {res['mmd2'][0]:.3e} floor {res['mmd2_floor'][0]:.3e} | energy "
        f"{res['energy'][0]:.3e} floor {res['energy_floor'][0]:.3e}")
  assert res["mmd2"][0] > 10.0 * abs(res["mmd2_floor"][0])
  assert res["energy"][0] > 10.0 * abs(res["energy_floor"][0])
