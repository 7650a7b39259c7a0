"""The fused sliced Wasserstein distance on the GPU: cnf_sliced_w2 / utils.sliced_wasserstein /
autograd.sliced_wasserstein / applications.sliced_loss_fn / solvers.evaluate_fp_sliced, against the float64 restatement
(tests/sliced_ref.py).

On the exact grid (sliced_ref.clouds_exact / directions_exact) every float32 key is exact under any operation order, so
the kernel and the restatement sort the same numbers by the same rule (key, then index) and must find the same
permutation: the values then agree to the rounding of double sums, 1e-12 relative, and N grad to the one rounding of the
stored float32 -- 4 of its ulps are allowed.  A mismatch there is a bug, not rounding.

The kernel's own boundaries, each with a shape below, at and above it (SHAPES; T = cnf_sliced_tile() keys per sorted
tile, read from the source at import): the lane's 16 keys (N, M = 15, 16, 17), the wave of 64 (63, 65; 129, 64), the 256
ranks per workgroup of sliced_w2_kernel (255, 256, 257), the tile (T - 1, T, T + 1: no merge pass / one), two merge
passes with a ragged last run (2 T + 1 against 3 T - 5), and overlap loops of 334 ranks on either side.

On ordinary Gaussian inputs the keys are rounded, and the torch float32 composition on the device -- a matrix product,
torch.sort, the merged-quantile sum -- is the yardstick: e_fused <= 2 e_composed + floor, the floor being the float32
rounding of a key carried into the quantity: value 8 * 2^-24 max|k| max|k - l|, N grad 8 * 2^-24 max|k| (N a is a
weighted mean of differences k - l, |theta| <= 1), from the restatement's numbers.  The gradient is compared on the rows
whose rank under every projection agrees between the restatement and the composition (the others sit within one
rounding of a neighbour and may swap); at most 1 % of the rows may be left out (tests/test_sliced_cpu.py checks the
seeds on the CPU).

The project's allocation probe (test_compute_calls_never_allocate) watches the model's table workspace, which a
model-free call does not have: the captured call below is the check that nothing is allocated (an allocation fails a
capture).

Measured on one MI355X (every test prints its figures: run with -s):
  the 21 exact-grid shapes, grouping, ties   values within 3.9e-16 relative (bar 1e-12), N grad within 0.97 float32 ulps (bar 4)
  ordinary D=2, N=2048, M=1500, P=8          values fused 1.4e-17 composed 6.5e-9 floor 1.9e-5 | N grad fused 2.9e-8 composed
                                             6.6e-8 floor 2.2e-6 | rows left out 0 %
  ordinary D=10                              values 2.8e-17 / 1.3e-8 / 2.1e-5 | N grad 7.4e-9 / 1.7e-8 / 2.3e-6 | rows left out 0 %
  translation on the grid, N = M = 4096      values 0.0 relative, N grad 3.9e-8 relative (bar 1e-6); w(x, x) and its gradient 0
  sliced_loss_fn, D = 2 / 3                  loss 1.9e-7 / 6.7e-8; parameter gradient 2.9e-6 / 3.4e-7 against flow_adjoint_f64.bound
                                             = 2.5e-5 / 9.9e-6; autograd.sliced_wasserstein(flow_forward(...)) gave the fast path's
                                             gradient bit for bit; no rank differed between the float32 and float64 flows
  evaluate_fp_sliced, 4096 per half          sw 0.65 .. 1.01 over a floor of 5.8e-4 .. 6.8e-4; the marginals' W2 floor 0.028 ..
                                             0.044 against the scale 0.017 .. 0.022
More cases: profiles/sliced/README.md.
"""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sliced_ref as sl

_SRC = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "cnf_ot_amd", "csrc", "cnf_sliced.hip")).read()
T = int(re.search(r"#define SL_TILE (\d+)", _SRC).group(1))
W = 64
# (D, N, M, P, S)
SHAPES = [(1, 1, 1, 1, 1), (2, 2, 3, 3, 1),
          (2, 15, 17, 2, 1), (2, 16, 15, 2, 1), (2, 17, 16, 2, 1),
          (2, W - 1, W + 1, 3, 2), (3, 2 * W + 1, W, 3, 1),
          (2, 255, 256, 2, 1), (2, 256, 257, 2, 1), (2, 257, 255, 2, 1),
          (2, T - 1, T, 2, 1), (2, T, T + 1, 2, 1), (2, T + 1, T - 1, 2, 1),
          (2, 2 * T + 1, 3 * T - 5, 2, 1),
          (2, 3, 1000, 2, 1), (2, 1000, 3, 2, 1),
          (1, 300, 257, 5, 1), (7, 300, 257, 5, 1), (10, 300, 257, 5, 1), (14, 300, 257, 5, 1),
          (2, 513, 130, 4, 3)]
_REF = {}


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def _ref(key, x, y, theta):
  """The restatement of one set, computed once per key and never changed"""
  if key not in _REF:
    _REF[key] = sl.run(x, y, theta)
  return _REF[key]


def _workspace(S, N, M, D, G, want_grad):
  from cnf_ot_amd import _capi
  nbytes = ctypes.c_int64(0)
  _capi.check(_capi.lib().cnf_sliced_workspace(S, N, M, D, G, int(want_grad), ctypes.byref(nbytes)), "cnf_sliced_workspace")
  return nbytes.value


def _call(dev, x, y, theta, G=None, grad=True, fill=None, stream=None, out=None, short=0, expect=0):
  """cnf_sliced_w2 through the C ABI on device tensors x [S, N, D], y [S, M, D], theta [P, D]: a dict of sums
  [S, P + 2] and grad [S, N, D] (None where not asked for).  short: bytes withheld from the workspace size passed"""
  from cnf_ot_amd import _capi
  from cnf_ot_amd.flows import _stream_ptr
  S, N, D = x.shape
  M, P = y.shape[1], theta.shape[0]
  G = P if G is None else G
  nbytes = _workspace(S, N, M, D, G, grad)
  if out is None:
    out = {"ws": torch.zeros(nbytes, dtype=torch.uint8, device=dev),
           "sums": torch.full((S, P + 2), 7.25, dtype=torch.float64, device=dev),
           "grad": torch.full((S, N, D), 7.25, dtype=torch.float32, device=dev) if grad else None}
  if fill is not None:
    out["ws"].fill_(fill)
  for t in (x, y, theta):
    assert t.is_contiguous() and t.dtype == torch.float32
  rc = _capi.lib().cnf_sliced_w2(S, x.data_ptr(), N, y.data_ptr(), M, D, theta.data_ptr(), P, G, out["sums"].data_ptr(),
                                 None if out["grad"] is None else out["grad"].data_ptr(), out["ws"].data_ptr(),
                                 nbytes - short, _stream_ptr(dev) if stream is None else stream)
  assert rc == expect, rc
  if stream is None:
    torch.cuda.synchronize()
  return out


def _to(dev, *arrays):
  return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


def _ulps32(v):
  return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def _check_exact(dev, x, y, theta, tag, key, G=None):
  """x [S, N, D], y [S, M, D] on the exact grid: sums to 1e-12 relative (+ 1e-300), N grad to 4 float32 ulps (+ 1e-30)"""
  S, N, _ = x.shape
  o = _call(dev, *_to(dev, x, y, theta), G=G)
  sums, grad = o["sums"].cpu().numpy(), o["grad"].double().cpu().numpy() * N
  worst_v = worst_g = 0.0
  for s in range(S):
    r = _ref(key + (s,), x[s], y[s], theta)
    e_v = np.abs(sums[s] - r["sums"])
    e_g = np.abs(grad[s] - r["grad"] * N)
    worst_v = max(worst_v, float((e_v / np.maximum(np.abs(r["sums"]), 1e-300)).max()))
    worst_g = max(worst_g, float((e_g / _ulps32(r["grad"] * N)).max()))
    assert (e_v <= 1e-12 * np.abs(r["sums"]) + 1e-300).all(), (tag, s, sums[s], r["sums"])
    assert (e_g <= 4.0 * _ulps32(r["grad"] * N) + 1e-30).all(), (tag, s, float(e_g.max()))
  print(f"\n[sliced exact {tag}] SW {float(sums[0, -2]):.6f}: values {worst_v:.1e} relative, N grad {worst_g:.2f} float32 ulps")
  return o


@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "D%d-N%d-M%d-P%d-S%d" % v)
def test_exact_grid_parity(dev, shape):
  D, N, M, P, S = shape
  index = SHAPES.index(shape)
  x, y = sl.clouds_exact(D, N, M, seed=100 + index, S=S)
  _check_exact(dev, x, y, sl.directions_exact(D, P, seed=index), "D=%d N=%d M=%d P=%d S=%d" % shape, ("exact", shape))


def test_the_boundaries_named_above_are_the_kernels():
  from cnf_ot_amd import _capi
  assert _capi.lib().cnf_sliced_tile() == T
  assert "SL_E = 16;" in _SRC and "SL_ROWS = 256;" in _SRC and "SL_THREADS = SL_T / SL_E;" in _SRC


def test_grouping_and_the_workspace_do_not_show(dev):
  D, N, M, P, S = 2, 2 * T + 1, 513, 7, 2
  x, y = sl.clouds_exact(D, N, M, seed=200, S=S)
  theta = sl.directions_exact(D, P, seed=200)
  base = _check_exact(dev, x, y, theta, "grouping G=7", ("grouping",), G=7)
  xd, yd, td = _to(dev, x, y, theta)
  for G in (1, 2, 3):
    for fill in (0x00, 0xFF):                             # (0xFF bytes: NaN wherever a word is read before it is written)
      o = _call(dev, xd, yd, td, G=G, fill=fill)
      assert torch.equal(o["sums"], base["sums"]) and torch.equal(o["grad"], base["grad"]), (G, fill)
  o = _call(dev, xd, yd, td, G=7, fill=0xFF)
  assert torch.equal(o["sums"], base["sums"]) and torch.equal(o["grad"], base["grad"])
  o = _call(dev, xd, yd, td, G=3, grad=False)             # the values do not depend on the gradient being asked for
  assert torch.equal(o["sums"], base["sums"])
  # one byte too few: refused, nothing written
  from cnf_ot_amd import _capi
  o = _call(dev, xd, yd, td, G=3, short=1, expect=_capi.CNF_ERR_INVALID)
  assert bool((o["sums"] == 7.25).all()) and bool((o["grad"] == 7.25).all()) and not bool(o["ws"].any())


def test_ties(dev):
  D, N, M, P = 2, 300, 257, 4
  x, y = sl.clouds_exact(D, N, M, seed=300)
  theta = sl.directions_exact(D, P, seed=300)
  xx = np.repeat(x, 2, axis=0)                            # every row twice: every key of x is tied with its neighbour's
  _check_exact(dev, xx[None], y[None], theta, "rows duplicated", ("ties", 0))
  same = np.repeat(x[:1], N, axis=0)                      # N identical points: the order is the index alone
  _check_exact(dev, same[None], y[None], theta, "identical points", ("ties", 1))
  _check_exact(dev, y[None], same[None], theta, "identical targets", ("ties", 2))


def _composed(xd, yd, td):
  """The torch float32 composition on the device for one set: (w [P], N grad [N, D], perm_x [P, N]) as numpy"""
  N, M = len(xd), len(yd)
  kx, ky = (xd @ td.T).T.contiguous(), (yd @ td.T).T.contiguous()
  sx, px = torch.sort(kx, dim=1, stable=True)
  sy, _ = torch.sort(ky, dim=1, stable=True)
  if N == M:
    diff = sx - sy
    w = 0.5 * (diff * diff).mean(1)
    a_rank = diff / N
  else:
    ix, iy, o = sl.segments(N, M)
    ix, iy = torch.from_numpy(ix).to(xd.device), torch.from_numpy(iy).to(xd.device)
    o = torch.from_numpy(o.astype(np.float32)).to(xd.device)
    diff = sx[:, ix] - sy[:, iy]
    w = 0.5 * (o * diff * diff).sum(1)
    a_rank = torch.zeros_like(sx).index_add_(1, ix, o * diff)
  a = torch.empty_like(a_rank).scatter_(1, px, a_rank)
  grad = (a[:, :, None] * td[:, None, :]).sum(0) / len(td)
  return w.double().cpu().numpy(), grad.double().cpu().numpy() * N, px.cpu().numpy()


@pytest.mark.parametrize("D", sorted(sl.ORDINARY))
def test_ordinary_inputs_against_the_composition(dev, D):
  from cnf_ot_amd import utils
  N, M, P, seed = sl.ORDINARY[D]
  x, y = sl.clouds(D, N, M, seed)
  theta = utils.sliced_directions(D, P, seed).numpy()
  r = _ref(("ordinary", D), x, y, theta)
  xd, yd, td = _to(dev, x, y, theta)
  o = _call(dev, xd[None], yd[None], td)
  g_w, g_g = o["sums"][0, :P].cpu().numpy(), o["grad"][0].double().cpu().numpy() * N
  c_w, c_g, c_perm = _composed(xd, yd, td)
  k_max = float(max(np.abs(r["kx"]).max(), np.abs(r["ky"]).max()))
  d_max = float(max(r["kx"].max() - r["ky"].min(), r["ky"].max() - r["kx"].min()))
  floor_v, floor_g = 8.0 * 2.0 ** -24 * k_max * d_max, 8.0 * 2.0 ** -24 * k_max
  keep = sl.rows_that_agree(r["perm_x"], c_perm)
  left_out = 1.0 - keep.mean()
  e_v, e_vc = np.abs(g_w - r["w"]).max(), np.abs(c_w - r["w"]).max()
  e_g, e_gc = np.abs(g_g - r["grad"] * N)[keep].max(), np.abs(c_g - r["grad"] * N)[keep].max()
  e_all = np.abs(g_g - r["grad"] * N).max()
  print(f"\n[sliced ordinary D={D}] SW {r['sw']:.6f}: values fused {e_v:.2e} composed {e_vc:.2e} floor {floor_v:.2e} | N grad fused "
        f"{e_g:.2e} (all rows {e_all:.2e}) composed {e_gc:.2e} floor {floor_g:.2e} | rows left out {100 * left_out:.3f} %")
  assert left_out <= 0.01
  assert e_v <= 2.0 * e_vc + floor_v and e_g <= 2.0 * e_gc + floor_g
  assert abs(float(o["sums"][0, P]) - r["sw"]) <= 2.0 * e_vc + floor_v
  assert abs(float(o["sums"][0, P + 1]) - r["max_sliced"]) <= 2.0 * e_vc + floor_v


def test_closed_forms_on_the_device(dev):
  from cnf_ot_amd import utils
  D, N, P = 3, 4096, 6
  x, _ = sl.clouds_exact(D, N, 1, seed=400)
  c = np.array([1.5, -0.75, 0.25], dtype=np.float32)
  theta = torch.from_numpy(sl.directions_exact(D, P, seed=4))        # (exact keys: what is left is the stored float32)
  res = utils.sliced_wasserstein(x, x + c, theta, want_grad=True)
  assert set(res) == {"sw", "per_projection", "max_sliced", "directions", "grad"}
  assert res["sw"].shape == (1,) and res["sw"].dtype == torch.float64 and res["per_projection"].shape == (1, P)
  assert res["grad"].shape == (N, D) and res["grad"].dtype == torch.float32 and res["directions"].shape == (P, D)
  tc = theta.numpy().astype(np.float64) @ c.astype(np.float64)
  want_w = 0.5 * tc * tc
  want_g = -(tc[:, None] * theta.numpy().astype(np.float64)).sum(0) / P
  e_w = float(np.abs(res["per_projection"][0].cpu().numpy() - want_w).max() / want_w.max())
  e_g = float(np.abs(res["grad"].double().cpu().numpy() * N - want_g[None, :]).max() / np.abs(want_g).max())
  print(f"\n[sliced translation N={N}] values {e_w:.2e} relative, N grad {e_g:.2e} relative (bar 1e-6)")
  assert e_w <= 1e-6 and e_g <= 1e-6
  assert abs(float(res["sw"][0]) - want_w.mean()) <= 1e-6 * want_w.max()
  assert abs(float(res["max_sliced"][0]) - want_w.max()) <= 1e-6 * want_w.max()
  # a cloud against itself, Gaussian: exactly 0, with a zero gradient
  g, _ = sl.clouds(D, N, 1, seed=401)
  same = utils.sliced_wasserstein(g, g.copy(), utils.sliced_directions(D, P, seed=4), want_grad=True)
  assert bool((same["per_projection"] == 0.0).all()) and float(same["sw"][0]) == 0.0 and bool((same["grad"] == 0.0).all())


def test_python_surface_equals_the_c_call(dev):
  from cnf_ot_amd import utils
  D, N, M, P, S = 3, 700, 1100, 5, 2
  x, y = sl.clouds(D, N, M, seed=500, S=S)
  theta = utils.sliced_directions(D, P, seed=5)
  xd, yd, td = _to(dev, x, y, theta.numpy())
  o = _call(dev, xd, yd, td)
  res = utils.sliced_wasserstein(xd.double(), y, theta, want_grad=True)     # float64 and host inputs are accepted
  assert torch.equal(res["per_projection"], o["sums"][:, :P]) and torch.equal(res["sw"], o["sums"][:, P])
  assert torch.equal(res["max_sliced"], o["sums"][:, P + 1]) and torch.equal(res["grad"], o["grad"])
  plain = utils.sliced_wasserstein(xd, yd, theta)
  assert plain["grad"] is None and torch.equal(plain["sw"], res["sw"])
  # the default directions: sliced_directions(D, n_proj, seed)
  d = utils.sliced_wasserstein(xd, yd, n_proj=5, seed=5)
  assert torch.equal(d["directions"].cpu(), theta) and torch.equal(d["sw"], res["sw"])
  # a small workspace limit means small groups, and the same bits
  G, nbytes = utils.sliced_group(S, N, M, D, P, True, limit=_workspace(S, N, M, D, 2, True))
  assert G == 2 and nbytes == _workspace(S, N, M, D, 2, True)
  assert utils.sliced_group(S, N, M, D, P, True)[0] == P and utils.sliced_group(S, N, M, D, P, True, limit=1)[0] == 1


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_non_finite_coordinate_stays_in_its_set(dev, bad):
  D, N, M, P, S = 2, 257, 130, 4, 3
  x, y = sl.clouds(D, N, M, seed=600, S=S)
  theta = sl.directions_exact(D, P, seed=600)
  xd, yd, td = _to(dev, x, y, theta)
  clean = _call(dev, xd, yd, td, G=2)
  for where in ("x", "y"):
    xb, yb = xd.clone(), yd.clone()
    (xb if where == "x" else yb)[1, 100, 1] = bad
    o = _call(dev, xb, yb, td, G=2)                       # (the call returns: every loop of the kernels is counted)
    assert bool(torch.isnan(o["sums"][1]).all()) and bool(torch.isnan(o["grad"][1]).all()), where
    for s in (0, 2):
      assert torch.equal(o["sums"][s], clean["sums"][s]) and torch.equal(o["grad"][s], clean["grad"][s]), (where, s)


def test_a_captured_call_replays_the_eager_bits(dev):
  D, N, M, P, S = 2, T + 300, 257, 5, 2
  x, y = sl.clouds(D, N, M, seed=700, S=S)
  theta = sl.directions_exact(D, P, seed=700)
  xd, yd, td = _to(dev, x, y, theta)
  eager = _call(dev, xd, yd, td, G=2)
  again = _call(dev, xd, yd, td, G=2)
  assert torch.equal(eager["sums"], again["sums"]) and torch.equal(eager["grad"], again["grad"])      # two calls: the same bits
  replay = _call(dev, xd, yd.flip(0).contiguous(), td, G=2)      # buffers of the same shapes, holding another call's numbers
  torch.cuda.synchronize()
  side = torch.cuda.Stream(device=dev)
  side.wait_stream(torch.cuda.current_stream(dev))
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side):              # (the call's launches are one linear chain; nothing is allocated)
    _call(dev, xd, yd, td, G=2, stream=side.cuda_stream, out=replay)
  for _ in range(2):
    for k in ("sums", "grad"):
      replay[k].fill_(7.25)
    graph.replay()
    torch.cuda.synchronize()
    for k in ("sums", "grad"):
      assert torch.isfinite(eager[k]).all() and torch.equal(eager[k], replay[k]), k


@pytest.mark.parametrize("D", [2, 3])
def test_training_term_against_the_float64_adjoint(dev, D):
  import sample_term_check
  from cnf_ot_amd import applications as app, autograd, utils
  B, M, P = 512, 384, 4
  _, tgt = sl.clouds(D, 2, M, seed=800 + D)
  theta = utils.sliced_directions(D, P, seed=8)

  def restate(out):      # (the envelope gradient)
    r = sl.run(out, tgt, theta.numpy())
    return r["sw"], r["grad"], r

  def floor(out64, runs):
    k_max = max(float(max(np.abs(r["kx"]).max(), np.abs(r["ky"]).max())) for r in runs)
    d_max = max(float(max(r["kx"].max() - r["ky"].min(), r["ky"].max() - r["kx"].min())) for r in runs)
    return 8.0 * 2.0 ** -24 * k_max * d_max

  def note(runs, runs32):
    swapped = sum(int((~sl.rows_that_agree(a["perm_x"], b["perm_x"])).sum()) for a, b in zip(runs, runs32))
    return f" | rows whose rank differs between the float32 and float64 flows: {swapped}"
  sample_term_check.check(dev, f"sliced_loss_fn D={D}", D, B, tgt, app.sliced_loss_fn, dict(directions=theta),
                          auto=lambda x, y: autograd.sliced_wasserstein(x, y, theta), restate=restate, floor=floor,
                          note=note, exact_autograd=True)


def test_evaluate_fp_sliced(dev):
  """The OU configuration, random parameters, 8 192 particles (4 096 per half).  The floor of w2_marginal is W2 between
  two independent empirical measures of n = 4 096 draws of the same one-dimensional Gaussian of deviation s_t
  (applications.ou_variance from the training's initial variance).  Quantile u of one sample has variance
  u (1 - u) / (n f(q_u)^2), the difference of two independent ones twice that, so
    E W2^2 = (2 / n) int u (1 - u) / f(q_u)^2 du = s_t^2 (2 / n) J_n,
  where J_n, the integral cut off at the extreme order statistics u = 1 / n, grows like log log n: between 1 and 3 for
  every n from 10^2 to 10^7.  The scale s_t sqrt(2 / n) is the J = 1 figure; 5 times it allows J up to 25."""
  from cnf_ot_amd import FlowConfig, Params, applications as app, solvers
  config = solvers.load_config(overrides={"general": {"type": "fp", "dim": 2}, "fp": {"velocity_field_type": "ou"}})
  model = solvers.build_model(config)
  params = Params.random(FlowConfig(dim=2), 0.2, seed=4, device=dev)
  n_particles = 8192
  res = solvers.evaluate_fp_sliced(config, model, params, n_particles=n_particles, h=1e-2, seed=5, n_proj=16)
  assert set(res) == set(solvers.FP_SLICED_KEYS)
  solvers.print_fp_sliced(res)
  S, f = len(res["times"]), config["fp"]
  assert S >= 2 and res["n"] == n_particles // 2 and res["n_proj"] == 16
  for k in ("sw", "sw_floor", "max_sliced", "max_sliced_floor", "w2_marginal", "w2_marginal_floor"):
    v = np.asarray(res[k], dtype=np.float64)
    assert v.shape == ((S, 2) if k.startswith("w2") else (S,)) and np.isfinite(v).all() and (v >= 0.0).all(), k
  for i, t in enumerate(res["times"]):
    assert res["sw_floor"][i] < res["sw"][i] <= res["max_sliced"][i]
    scale = math.sqrt(app.ou_variance(t, f["a"], app.fp_initial_variance(f["T"]), f["sigma"])) * math.sqrt(2.0 / res["n"])
    print(f"[evaluate_fp_sliced t={t:.3f}] floor of the marginals' W2 {res['w2_marginal_floor'][i]} against the scale {scale:.3e}")
    assert max(res["w2_marginal_floor"][i]) < 5.0 * scale
