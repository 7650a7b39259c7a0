"""The fused kernel Stein discrepancy on the GPU: cnf_stein / utils.ksd / autograd.ksd / applications.ksd_loss_fn /
applications.mv_stationary_score / solvers.evaluate_ksd, against the float64 restatement (tests/stein_ref.py), with the
same composition in float32 -- pair matrices in float32, reduced in float64 -- as the yardstick of the fused error, the
project's bar (test_gpu_interaction.py):
  e_fused <= 2 e_composed + 4 EPS scale,   EPS = 5e-6,
scale = the largest per-pair sum of the absolute values of the summands: the four terms of k_p for the pair mean of
sums and for rows, the per-pair gradient contribution per component for grad_x and grad_score (both as pair means:
the outputs times N / 2).  The kernel's float32 accumulators live for one tile of IA_TILE = 64 columns (64 * 2^-24 =
3.8e-6 of the tile's largest term times its length); per-pair rounding (differences, the fmaf chains, one v_log_f32 +
v_exp_f32 + v_rcp_f32 or one v_exp_f32 per term, three or four fmaf into the sums) stays below 1e-6 of the summands.
Scores are of size |x| (s = -x + 0.3 noise), so that s . s phi cancels against the other terms as it does in use.

The kernel's own boundaries, each with a shape below, at and above it: IA_TILE = 64 columns (N = 63, 64, 65); the rows of
one workgroup, 256 lanes x st_rows(D) = 512 for D <= 8 (N = 511, 512, 513) and 256 above (D = 10: N = 255, 256, 257);
more than one row group AND more than one split: (3, 1030), (10, 300), (14, 300) (asserted below).

Every test prints its figures (run with -s); the worst share of the bar measured on one MI355X is in DESIGN.md 5.3q.
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
import stein_ref as sr

EPS = 5e-6
SHAPES = [(1, 2), (1, 700), (2, 63), (2, 64), (2, 65), (2, 511), (2, 512), (2, 513), (3, 257), (3, 1030),
          (10, 255), (10, 256), (10, 257), (10, 300), (14, 129), (14, 300)]                    # (D, N)


def _specs(D):
  r = float(np.sqrt(D))
  return {"imq/1": sr.spec("imq", [r]),
          "imq/4": sr.spec("imq", [0.5 * r, r, 2.0 * r, 4.0 * r], [1.0, 0.5, 0.25, 0.75], beta=-0.75),
          "gaussian/1": sr.spec("gaussian", [r]),
          "gaussian/4": sr.spec("gaussian", [0.5 * r, r, 2.0 * r, 4.0 * r], [1.0, 0.5, 0.25, 0.75])}


SPEC_NAMES = list(_specs(1))


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def _inputs(D, N, index, S=None):
  """(x, s) float32: a Gaussian cloud and a score of its size"""
  x = sr.cloud(D, N, 5000 + index, scale=1.0 + 0.125 * (index % 5), S=S)
  s = (-x + np.float32(0.3) * sr.cloud(D, N, 6000 + index, S=S)).astype(np.float32)
  return x, s


@functools.lru_cache(maxsize=None)
def _reference(D, N, index, name):
  """The restatement of one (shape, spec) case and its float32 composition, computed once"""
  x, s = _inputs(D, N, index)
  sp = _specs(D)[name]
  return sr.stats(x, s, sp), sr.stats(x, s, sp, dtype=np.float32)


def _call(dev, x, s, sp, want_rows=True, want_grad=True, fill=None, stream=None, out=None):
  """cnf_stein through the C ABI on device tensors x, s [S, N, D]: (sums [S, 2], rows [S, N] or None, grad_x, grad_s
  [S, N, D] or None, workspace).  out: a former result to write into (nothing is allocated, nothing waited for)."""
  from cnf_ot_amd import _capi, utils
  from cnf_ot_amd.flows import _stream_ptr
  spec = utils.stein_spec(**sr.kwargs(sp))
  S, N, D = x.shape
  lib = _capi.lib()
  nbytes = ctypes.c_int64(0)
  _capi.check(lib.cnf_stein_workspace(S, N, D, int(want_grad), ctypes.byref(nbytes)), "cnf_stein_workspace")
  if out is None:
    ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
    if fill is not None:
      ws.fill_(fill)
    sums = torch.empty(S, 2, dtype=torch.float64, device=dev)
    rows = torch.empty(S, N, dtype=torch.float32, device=dev) if want_rows else None
    gx = torch.empty(S, N, D, dtype=torch.float32, device=dev) if want_grad else None
    gs = torch.empty(S, N, D, dtype=torch.float32, device=dev) if want_grad else None
  else:
    sums, rows, gx, gs, ws = out
  assert x.is_contiguous() and s.is_contiguous() and x.dtype == s.dtype == torch.float32 and x.shape == s.shape
  ptr = lambda t: None if t is None else t.data_ptr()
  _capi.check(lib.cnf_stein(ctypes.byref(spec), S, x.data_ptr(), s.data_ptr(), N, D, sums.data_ptr(), ptr(rows), ptr(gx),
                            ptr(gs), ws.data_ptr(), nbytes.value, _stream_ptr(dev) if stream is None else stream),
              "cnf_stein")
  if out is None:
    torch.cuda.synchronize()
  return sums, rows, gx, gs, ws


def _same(a, b):
  return all((u is None and v is None) or torch.equal(u, v) for u, v in zip(a[:4], b[:4]))


SHARES = {}


def _check(got, ref, comp, N, tag):
  """One set's (sums [2], rows [N], grad_x, grad_s [N, D]) against the restatement under the bar above"""
  n64 = lambda t: t.cpu().double().numpy()
  pairs = N * (N - 1.0)
  rows, gx, gs = n64(got[1]), n64(got[2]), n64(got[3])
  half = 0.5 * N                                  # (the gradients as pair means)
  e = {"sum": (abs(float(got[0][0]) - ref["sums"][0]) / pairs, abs(comp["sums"][0] - ref["sums"][0]) / pairs, ref["scale_v"]),
       "diag": (abs(float(got[0][1]) - ref["sums"][1]) / N, 0.0, abs(ref["sums"][1]) / N),
       "rows": (np.abs(rows - ref["rows"]).max(), np.abs(comp["rows"] - ref["rows"]).max(), ref["scale_v"]),
       "grad_x": (half * np.abs(gx - ref["grad_x"]).max(), half * np.abs(comp["grad_x"] - ref["grad_x"]).max(), ref["scale_gx"]),
       "grad_s": (half * np.abs(gs - ref["grad_s"]).max(), half * np.abs(comp["grad_s"] - ref["grad_s"]).max(), ref["scale_gs"])}
  print(f"\n[stein {tag}] ksd2 {ref['sums'][0] / pairs:+.6f} | " + " | ".join(
    f"{k}: fused {a:.2e} composed {b:.2e} floor {4 * EPS * c:.2e}" for k, (a, b, c) in e.items()))
  assert np.isfinite(float(got[0][0])) and np.isfinite(rows).all() and np.isfinite(gx).all() and np.isfinite(gs).all()
  for k, (a, b, c) in e.items():
    bar = 2.0 * b + 4.0 * EPS * c
    SHARES[k] = max(SHARES.get(k, 0.0), a / bar if bar > 0.0 else 0.0)
    assert a <= bar, (tag, k, a, b, c)


@pytest.mark.parametrize("name", SPEC_NAMES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "D%d-N%d" % s)
def test_value_rows_and_gradients_against_the_restatement(dev, shape, name):
  D, N = shape
  index = SHAPES.index(shape)
  x, s = _inputs(D, N, index)
  sp = _specs(D)[name]
  ref, comp = _reference(D, N, index, name)
  xd, sd = torch.from_numpy(x).to(dev)[None], torch.from_numpy(s).to(dev)[None]
  got = _call(dev, xd, sd, sp)
  # sums are the same bits whatever else is asked for, and so are the rows
  for wr, wg in ((False, False), (True, False), (False, True)):
    other = _call(dev, xd, sd, sp, want_rows=wr, want_grad=wg)
    assert torch.equal(got[0], other[0]) and (other[1] is None or torch.equal(other[1], got[1]))
    assert other[2] is None or (torch.equal(other[2], got[2]) and torch.equal(other[3], got[3]))
  _check((got[0][0], got[1][0], got[2][0], got[3][0]), ref, comp, N, f"{name} D={D} N={N}")
  print(f"[stein] worst shares of the bar so far: " + " ".join(f"{k} {v:.3f}" for k, v in SHARES.items()))


def test_the_boundaries_named_above_are_the_kernels(dev):
  from cnf_ot_amd import _capi
  lib = _capi.lib()
  assert lib.cnf_stein_splits(1, 64, 2) == 1 and lib.cnf_stein_splits(1, 65, 2) == 2
  assert lib.cnf_stein_splits(1, 512, 2) == 8 and lib.cnf_stein_splits(1, 513, 2) == 9
  assert lib.cnf_stein_splits(1, 256, 10) == 4 and lib.cnf_stein_splits(1, 257, 10) == 5
  for D, N in ((3, 1030), (10, 300), (14, 300)):      # more than one row group and more than one split
    R = 2 if D <= 8 else 1
    assert -(-N // (256 * R)) >= 2 and lib.cnf_stein_splits(1, N, D) >= 2
  assert lib.cnf_stein_splits(3, 1030, 2) >= 2 and lib.cnf_stein_splits(0, 8, 2) < 0 and lib.cnf_stein_splits(1, 8, 15) < 0
  here = os.path.join(os.path.dirname(_capi.__file__), "csrc")
  src = open(os.path.join(here, "cnf_stein.hip")).read()
  pairs = open(os.path.join(here, "cnf_interaction_pairs.h")).read()
  assert "ST_THREADS = IA_THREADS;" in src and "ST_R_MAX_D = 8;" in src and "return D <= ST_R_MAX_D ? 2 : 1;" in src
  assert "IA_THREADS = 256;" in pairs and "IA_TILE = 64;" in pairs


def test_the_c_abi_refuses_before_any_launch(dev):
  from cnf_ot_amd import _capi, utils
  lib = _capi.lib()
  x = torch.zeros(1, 8, 2, device=dev)
  sums = torch.full((1, 2), 7.0, dtype=torch.float64, device=dev)
  ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
  g = torch.zeros(1, 8, 2, device=dev)

  def rc(spec, S=1, N=8, D=2, gx=None, gs=None, nbytes=1 << 16):
    return lib.cnf_stein(ctypes.byref(spec), S, x.data_ptr(), x.data_ptr(), N, D, sums.data_ptr(), None, gx, gs, ws.data_ptr(),
                         nbytes, None)
  good = utils.stein_spec("imq", [1.0])

  def bad(**kw):
    sp = utils.stein_spec("imq", [1.0, 2.0])
    for k, v in kw.items():
      if isinstance(v, tuple):
        getattr(sp, k)[v[0]] = v[1]
      else:
        setattr(sp, k, v)
    return sp
  inf, nan = float("inf"), float("nan")
  specs = [bad(kind=0), bad(kind=3), bad(n_terms=0), bad(n_terms=5), bad(w=(1, 0.0)), bad(w=(1, -1.0)), bad(w=(0, inf)),
           bad(w=(0, nan)), bad(bw=(1, 0.0)), bad(bw=(0, -1.0)), bad(bw=(0, inf)), bad(bw=(0, nan)), bad(beta=0.0),
           bad(beta=-1.0), bad(beta=nan), bad(bw=(0, 1e-9)), bad(bw=(0, 1e25)), bad(w=(0, 3e38)),
           bad(kind=2, bw=(0, 1e-7))]
  for sp in specs:
    assert rc(sp) == _capi.CNF_ERR_INVALID
  for kw in (dict(S=0), dict(S=65), dict(N=1), dict(N=(1 << 20) + 1), dict(D=0), dict(D=15), dict(gx=g.data_ptr()),
             dict(gs=g.data_ptr()), dict(nbytes=8)):
    assert rc(good, **kw) == _capi.CNF_ERR_INVALID
  torch.cuda.synchronize()
  assert float(sums[0, 0]) == 7.0                 # nothing was enqueued
  assert rc(good) == _capi.CNF_OK
  torch.cuda.synchronize()
  assert float(sums[0, 0]) != 7.0


@pytest.mark.parametrize("name", SPEC_NAMES)
def test_three_sets_with_their_own_data(dev, name):
  D, N, S = 2, 257, 3
  x, s = _inputs(D, N, 40, S=S)
  x[1] *= np.float32(1.25)                               # (the sets differ in law as well as in draw)
  sp = _specs(D)[name]
  got = _call(dev, torch.from_numpy(x).to(dev), torch.from_numpy(s).to(dev), sp)
  for k in range(S):
    _check((got[0][k], got[1][k], got[2][k], got[3][k]), sr.stats(x[k], s[k], sp), sr.stats(x[k], s[k], sp, dtype=np.float32),
           N, f"S=3 set {k} {name}")
  assert len({round(float(v) / (N * N), 6) for v in got[0][:, 0]}) == S      # three different numbers: no set read twice


@pytest.mark.parametrize("name", ["imq/4", "gaussian/4"])
@pytest.mark.parametrize("D", [3, 10])
def test_reproducibility(dev, name, D):
  N, S = 700, 2
  x, s = _inputs(D, N, 41, S=S)
  sp = _specs(D)[name]
  xd, sd = torch.from_numpy(x).to(dev), torch.from_numpy(s).to(dev)
  base = _call(dev, xd, sd, sp)
  assert _same(base, _call(dev, xd, sd, sp))                          # two calls
  assert _same(base, _call(dev, xd, sd, sp, fill=0xFF))               # (0xFF bytes: NaN doubles wherever a word is read unwritten)
  # one call replayed from a captured graph: a single stream, one linear chain of launches, nothing allocated
  replay = _call(dev, xd.flip(1).contiguous(), sd.flip(1).contiguous(), sp)
  torch.cuda.synchronize()
  side = torch.cuda.Stream(device=dev)
  side.wait_stream(torch.cuda.current_stream(dev))
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side):
    _call(dev, xd, sd, sp, stream=side.cuda_stream, out=replay)
  for t in replay[:4]:
    t.fill_(7)
  graph.replay()
  torch.cuda.synchronize()
  assert _same(base, replay)


@pytest.mark.parametrize("name", ["imq/1", "gaussian/4"])
def test_coincident_points(dev, name):
  D, N = 3, 150
  x, s = _inputs(D, N, 44)
  x[100:120], s[100:120] = x[:20], s[:20]                 # duplicated rows: they interact (k_p(x, x) off the diagonal)
  sp = _specs(D)[name]
  got = _call(dev, torch.from_numpy(x).to(dev)[None], torch.from_numpy(s).to(dev)[None], sp)
  _check((got[0][0], got[1][0], got[2][0], got[3][0]), sr.stats(x, s, sp), sr.stats(x, s, sp, dtype=np.float32), N,
         f"{name}, coincident points")
  # equal points, equal rows: the same pairs in another order of the float32 tiles
  assert float((got[1][0, 100:120] - got[1][0, :20]).abs().max()) <= 4.0 * EPS * sr.stats(x, s, sp)["scale_v"]
  # all points coincident: every pair is the diagonal's value, k_p(x, x) = phi(0) |s|^2 - 2 D phi'(0)
  x1, s1 = np.tile(x[:1], (70, 1)), np.tile(s[:1], (70, 1))
  one = _call(dev, torch.from_numpy(x1).to(dev)[None], torch.from_numpy(s1).to(dev)[None], sp)
  assert all(torch.isfinite(t).all() for t in one[:4])
  ref = sr.stats(x1, s1, sp)
  assert abs(float(one[0][0, 0]) - ref["sums"][0]) <= 4.0 * EPS * ref["scale_v"] * 70 * 69
  assert abs(float(one[0][0, 0]) / 69.0 - float(one[0][0, 1])) <= 4.0 * EPS * ref["scale_v"] * 70


def test_far_clusters_underflow_to_exactly_zero(dev):
  D, N = 3, 300
  x, s = _inputs(D, N, 42)
  x[150:] += np.float32(1000.0)
  sp = sr.spec("gaussian", [0.1])
  xd, sd = torch.from_numpy(x).to(dev), torch.from_numpy(s).to(dev)
  whole = _call(dev, xd[None], sd[None], sp)
  assert all(torch.isfinite(t).all() for t in whole[:4])
  # the cross-cluster pairs contribute exactly 0: each point's row sum is its own cluster's
  a = _call(dev, xd[None, :150].contiguous(), sd[None, :150].contiguous(), sp)
  b = _call(dev, xd[None, 150:].contiguous(), sd[None, 150:].contiguous(), sp)
  ref = sr.stats(x, s, sp)
  parts = sr.stats(x[:150], s[:150], sp)["sums"][0] + sr.stats(x[150:], s[150:], sp)["sums"][0]
  assert ref["sums"][0] == parts or abs(ref["sums"][0] - parts) <= 1e-12 * abs(parts)
  floor = 4.0 * EPS * ref["scale_v"]
  assert abs(float(whole[0][0, 0]) - float(a[0][0, 0]) - float(b[0][0, 0])) <= floor * N * (N - 1)
  rows = torch.cat([a[1][0], b[1][0]]).double() * (149.0 / 299.0)
  assert float((whole[1][0].double() - rows).abs().max()) <= floor
  assert float((whole[2][0].double() * (N * (N - 1.0)) - torch.cat([a[2][0], b[2][0]]).double() * (150.0 * 149.0)).abs().max()) \
      <= 2.0 * 4.0 * EPS * ref["scale_gx"] * (N - 1)


def test_a_nan_stays_in_its_own_set(dev):
  D, N, S = 2, 300, 3
  x, s = _inputs(D, N, 47, S=S)
  sp = _specs(D)["imq/4"]
  xd, sd = torch.from_numpy(x).to(dev), torch.from_numpy(s).to(dev)
  base = _call(dev, xd, sd, sp)
  for which in (xd, sd):
    bad = which.clone()
    bad[1, 77, 1] = float("nan")
    got = _call(dev, bad if which is xd else xd, bad if which is sd else sd, sp)
    for k in (0, 2):
      assert all(torch.equal(u[k], v[k]) for u, v in zip(base[:4], got[:4]))
    assert torch.isnan(got[0][1, 0]) and torch.isnan(got[1][1]).all() and torch.isnan(got[2][1]).any()
  inf = xd.clone()
  inf[1, 5, 0] = float("inf")
  got = _call(dev, inf, sd, sp)
  assert all(torch.equal(u[k], v[k]) for u, v in zip(base[:4], got[:4]) for k in (0, 2))


@pytest.mark.parametrize("name", ["imq/4", "gaussian/1"])
def test_the_python_surface(dev, name):
  from cnf_ot_amd import utils
  D, N, S = 2, 257, 3
  x, s = _inputs(D, N, 46, S=S)
  sp = _specs(D)[name]
  kw = sr.kwargs(sp)
  a = utils.ksd(x[0], s[0], want_grad=True, want_rows=True, **kw)
  b = utils.ksd(torch.from_numpy(x).to(dev).double(), torch.from_numpy(s).to(dev).double(), **kw)
  keys = {"ksd2", "ksd2_v", "sums", "rows", "grad_x", "grad_score", "direction", "bandwidths"}
  assert set(a) == set(b) == keys and b["rows"] is None and b["grad_x"] is None and b["direction"] is None
  assert a["ksd2"].shape == (1,) and a["ksd2"].dtype == torch.float64 and a["sums"].shape == (1, 2) and b["ksd2"].shape == (S,)
  assert a["rows"].shape == (N,) and a["grad_x"].shape == a["grad_score"].shape == a["direction"].shape == (N, D)
  xd, sd = torch.from_numpy(x).to(dev), torch.from_numpy(s).to(dev)
  one = _call(dev, xd[:1].contiguous(), sd[:1].contiguous(), sp)
  assert torch.equal(a["sums"], one[0]) and torch.equal(a["rows"], one[1][0]) and torch.equal(a["grad_x"], one[2][0])
  assert torch.equal(a["grad_score"], one[3][0])
  assert torch.equal(b["sums"], _call(dev, xd, sd, sp)[0])
  # (one float64 division each, on the device: the last bit may differ from the host's)
  u, v = float(one[0][0, 0]) / (N * (N - 1.0)), (float(one[0][0, 0]) + float(one[0][0, 1])) / (float(N) * N)
  assert abs(float(a["ksd2"][0]) - u) <= 2.0 ** -51 * abs(u) and abs(float(a["ksd2_v"][0]) - v) <= 2.0 ** -51 * abs(v) and v >= 0.0
  ref = sr.stats(x[0], s[0], sp)
  e = float(np.abs(a["direction"].cpu().double().numpy() - ref["direction"]).max())
  print(f"[stein direction {name}] error {e:.2e} floor {4 * EPS * ref['scale_gs']:.2e}")
  assert e <= 2.0 * np.abs(sr.stats(x[0], s[0], sp, dtype=np.float32)["direction"] - ref["direction"]).max() + 4.0 * EPS * ref["scale_gs"]
  # the default bandwidths: the median heuristic of x, its first four
  c = utils.ksd(x[0], s[0])
  assert c["bandwidths"] == [float(np.float32(v)) for v in utils.median_bandwidths(torch.from_numpy(x[0]))[:4]]


def test_autograd_in_x_and_in_the_score(dev):
  from cnf_ot_amd import autograd
  D, N, S = 3, 300, 2
  x, s = _inputs(D, N, 48, S=S)
  sp = _specs(D)["imq/4"]
  xt = torch.from_numpy(x).to(dev).requires_grad_(True)
  st = torch.from_numpy(s).to(dev).requires_grad_(True)
  val = autograd.ksd(xt, st, **sr.kwargs(sp))
  assert val.shape == (S,) and val.dtype == torch.float64
  w = torch.tensor([1.0, -2.5], dtype=torch.float64, device=dev)
  (val * w).sum().backward()
  for k in range(S):
    ref, comp = sr.stats(x[k], s[k], sp), sr.stats(x[k], s[k], sp, dtype=np.float32)
    for got, key, sc in ((xt.grad[k], "grad_x", "scale_gx"), (st.grad[k], "grad_s", "scale_gs")):
      e = 0.5 * N * np.abs(got.cpu().double().numpy() / float(w[k]) - ref[key]).max()
      assert e <= 2.0 * 0.5 * N * np.abs(comp[key] - ref[key]).max() + 4.0 * EPS * ref[sc], (k, key, e)
  only_x = autograd.ksd(xt.detach().requires_grad_(True), st.detach(), **sr.kwargs(sp))
  assert torch.equal(only_x.detach(), val.detach())


def test_a_score_chained_through_autograd_against_finite_differences(dev):
  from cnf_ot_amd import applications as app, autograd
  D, N = 2, 200
  x, _ = _inputs(D, N, 49)
  sp = _specs(D)["imq/1"]
  tgt = app.GaussianMixtureTarget([[0.5, -0.25], [-1.0, 0.75]], np.array([[1.5, 0.3], [0.3, 0.8]]), [0.4, 0.6])
  xt = torch.from_numpy(x).to(dev).requires_grad_(True)
  val = autograd.ksd(xt, tgt.score(xt), **sr.kwargs(sp))
  val.sum().backward()
  f = lambda pts: sr.ksd2(pts, tgt.score(torch.from_numpy(pts)).numpy(), sp)[0]
  x64 = x.astype(np.float64)
  ref = sr.stats(x64, tgt.score(torch.from_numpy(x64)).numpy(), sp)
  assert abs(float(val.detach()[0]) - f(x64)) <= 4.0 * EPS * ref["scale_v"] + 1e-6 * ref["scale_v"]   # (the float32 score: 2^-24 |s|)
  got = xt.grad.cpu().double().numpy()
  h = 1e-5
  worst = 0.0
  for (i, d) in [(0, 0), (7, 1), (63, 0), (64, 1), (199, 0)]:
    up, dn = x64.copy(), x64.copy()
    up[i, d] += h
    dn[i, d] -= h
    fd = (f(up) - f(dn)) / (2.0 * h)
    worst = max(worst, 0.5 * N * abs(got[i, d] - fd))
  # per pair: grad_x's own floor, and the score's Jacobian times grad_score's: |J| <= |P| + |P dmu|^2 / 4 with P = cov^-1
  # (|P| = 1.45) and dmu the distance of the two means (|P dmu| <= 2.7), so |J| <= 3.3; the differences add 1e-9 N / 2
  floor = 4.0 * EPS * (ref["scale_gx"] + 3.3 * ref["scale_gs"]) + 0.5 * N * 1e-9
  print(f"[stein chained score] worst pair-mean error against central differences {worst:.2e} (floor {floor:.2e})")
  assert worst <= floor


def test_a_shifted_target_stands_out(dev):
  """D = 2, N = 2048 exact N(0, I) draws (stein_ref.cloud, seed 100): KSD^2_U against their own score -x and against the
  score of N(0.5 1, I).  tests/stein_ref.py in float64 gives, for seeds 100 / 101 / 102, matched +1.06e-3 / -1.28e-4 /
  +1.02e-3 and shifted 0.248 / 0.288 / 0.301: ratios 233 / 2240 / 293 (seed 100, the one used: 233); the assertion asks
  for 20."""
  from cnf_ot_amd import utils
  x = sr.cloud(2, 2048, 100)
  sp = sr.spec("imq", [1.0])
  res = utils.ksd(np.stack([x, x]), np.stack([-x, -(x - np.float32(0.5))]), **sr.kwargs(sp))["ksd2"]
  matched, shifted = float(res[0]), float(res[1])
  print(f"[stein statistics] matched {matched:+.4e} shifted {shifted:+.4e} ratio {shifted / abs(matched):.1f}")
  assert shifted > 20.0 * abs(matched)


def _quadratic_ou():
  return dict(a=1.0, sigma=0.5, subtype="ou", interaction={"kind": "quadratic", "amplitudes": [0.75]}, strength=2.0)


def test_the_stationary_score_of_ou_with_the_quadratic_kernel(dev):
  from cnf_ot_amd import applications as app
  N, D = 600, 3
  x, _ = _inputs(D, N, 50, S=2)
  p = _quadratic_ou()
  got = app.mv_stationary_score(torch.from_numpy(x).to(dev), **p).cpu().double().numpy()
  x64 = x.astype(np.float64)
  lam = p["strength"] * 0.75 * N / (N - 1.0)      # (the force is a mean over the OTHER N - 1 points)
  want = -(p["a"] * x64 + lam * (x64 - x64.mean(1, keepdims=True))) / p["sigma"]
  e = np.abs(got - want).max()
  print(f"[mv_stationary_score] error {e:.2e} at |s| {np.abs(want).max():.2f}")
  assert e <= 4.0 * EPS * np.abs(want).max()
  xt = torch.from_numpy(x[0]).to(dev).requires_grad_(True)      # differentiable: d sum(s) / dx = -(a + lam (1 - 1 / N)) / sigma
  app.mv_stationary_score(xt, **p).sum().backward()
  assert float((xt.grad + p["a"] / p["sigma"]).abs().max()) <= 1e-4


def test_the_stationarity_residual_orders_the_two_laws(dev):
  """ou + quadratic (a = 1, sigma = 0.5, strength 2, amp 0.75), D = 2, N = 2048 draws z of stein_ref.cloud(seed 200):
  sqrt(sigma / (a + strength amp)) z, the interacting stationary law, against sqrt(sigma / a) z, the free one, both
  under mv_stationary_score at their own points.  tests/stein_ref.py in float64 gives, for seeds 200 / 201 / 202,
  stationary -4.50e-3 / -1.83e-3 / -3.42e-3 and free 0.653 / 0.705 / 0.724: ratios 145 / 386 / 212 (seed 200, the one
  used: 145); the assertion asks for 20."""
  from cnf_ot_amd import applications as app, utils
  p = _quadratic_ou()
  z = sr.cloud(2, 2048, 200)
  lam = p["a"] + p["strength"] * 0.75
  sets = torch.from_numpy(np.stack([np.float32(np.sqrt(p["sigma"] / lam)) * z, np.float32(np.sqrt(p["sigma"] / p["a"])) * z])).to(dev)
  res = utils.ksd(sets, app.mv_stationary_score(sets, **p), "imq", [1.0])["ksd2"]
  stat, free = float(res[0]), float(res[1])
  print(f"[stein stationarity] stationary {stat:+.4e} free {free:+.4e} ratio {free / abs(stat):.1f}")
  assert free > 20.0 * abs(stat)


@pytest.mark.parametrize("D", [2, 10])
def test_training_term_against_the_float64_adjoint(dev, D):
  import sample_term_check
  from cnf_ot_amd import applications as app, autograd
  B = 96
  sp = _specs(D)["imq/4"]
  kw = sr.kwargs(sp)
  mu, var = 0.5, 1.5
  tgt = app.GaussianMixtureTarget(np.full((1, D), mu), var)
  none = np.zeros((1, D), dtype=np.float32)      # (the shared harness hands every term a target set: this one has none)

  def restate(out):                               # the score of N(mu 1, var I) and its Jacobian -I / var
    r = sr.stats(out, -(out - mu) / var, sp)
    return r["sums"][0] / (len(out) * (len(out) - 1.0)), r["grad_x"] - r["grad_s"] / var, r
  sample_term_check.check(
      dev, f"ksd_loss_fn D={D}", D, B, none,
      lambda model, dim, params, _, cond, rng, batch, **k: app.ksd_loss_fn(model, dim, params, tgt, cond, rng, batch, **k),
      kw, auto=lambda x, y: autograd.ksd(x, tgt.score(x), **kw), restate=restate,
      floor=lambda out64, runs: 4.0 * EPS * max(r["scale_v"] for r in runs))


def test_it_trains(dev):
  from cnf_ot_amd import applications as app, solvers
  dim, B, rng = 2, 512, 3
  config = solvers.load_config(overrides={"general": {"dim": dim}})
  model = solvers.build_model(config)
  params = model.init(0)
  tgt = app.GaussianMixtureTarget([[1.0, -0.5]], 0.5)
  loss_fn = lambda p, r, _lambda, batch, grad=None: app.ksd_loss_fn(model, dim, p, tgt, [0.5], r, batch, "imq", [1.0], grad=grad)
  opt = solvers.Adam(1e-3)
  state = opt.init(params)
  update = solvers.make_update(loss_fn, opt, B)
  before = float(loss_fn(params, rng, 0.0, B))
  for _ in range(20):
    _, params, state = update(params, rng, 0.0, state)
  after = float(loss_fn(params, rng, 0.0, B))
  print(f"[ksd, 20 Adam steps towards N((1, -0.5), 0.5 I)] KSD^2_U {before:.6f} -> {after:.6f}")
  assert after < before


def test_evaluate_ksd_equals_its_composition(dev):
  from cnf_ot_amd import FlowConfig, Params, applications as app, solvers, utils
  dim, n, seed = 2, 1024, 5
  ia = {"kind": "quadratic", "strength": 2.0, "amplitudes": [0.75], "role": "drift"}
  config = solvers.load_config(overrides={"general": {"type": "fp", "dim": dim}, "fp": {"velocity_field_type": "ou"},
                                          "interaction": ia})
  model = solvers.build_model(config)
  params = Params.random(FlowConfig(dim=dim), 0.2, seed=4, device=dev)
  res = solvers.evaluate_ksd(config, model, params, n=n, seed=seed)
  assert set(res) == set(solvers.KSD_KEYS) and res["n"] == n and res["kind"] == "imq"
  entries = app.known_densities(config)
  assert res["times"] == [float(e[0]) for e in entries] and len(res["times"]) >= 2
  f = config["fp"]
  pos = app.fp_reference_particles(dim, f["T"], f["a"], f["sigma"], f["velocity_field_type"], res["times"], n, 1e-3, seed,
                                   positions=True)["pos"].float()
  for i, (t, target, scale) in enumerate(entries):
    x = model.apply.sample(params, cond=float(t), seed=seed, sample_shape=(n,)).float()
    exact = solvers.target_draws(target, scale, n, seed).to(dev)
    bw = utils.median_bandwidths(exact)[:4]
    both = utils.ksd(torch.stack([x, exact]), torch.stack([target.score(x, scale), target.score(exact, scale)]), "imq", bw)["ksd2"]
    assert res["flow"][i] == float(both[0]) and res["floor"][i] == float(both[1])
    bw = utils.median_bandwidths(pos[i])[:4]
    assert res["ensemble"][i] == float(utils.ksd(pos[i], target.score(pos[i], scale), "imq", bw)["ksd2"][0])
    both = utils.ksd(torch.stack([pos[i], x]), torch.stack([model.apply.score(params, pos[i].contiguous(), cond=float(t)),
                                                            model.apply.score(params, x.contiguous(), cond=float(t))]), "imq", bw)["ksd2"]
    assert res["ensemble_flow"][i] == float(both[0]) and res["flow_own"][i] == float(both[1])
  st = res["stationary"]
  assert set(st) == {"flow", "particles"} and len(st["particles"]) == 2 and all(np.isfinite(v) for v in st["particles"])
  solvers.print_ksd(res)
  # another type: no ensemble columns, no residual
  ot = solvers.evaluate_ksd(solvers.load_config(overrides={"general": {"type": "ot", "dim": dim}}), model, params, n=n, seed=seed)
  assert ot["ensemble"] is None and ot["stationary"] is None and len(ot["flow"]) == len(ot["times"]) == 2
  solvers.print_ksd(ot)
