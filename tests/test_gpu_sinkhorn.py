"""The fused Sinkhorn divergence on the GPU: cnf_sinkhorn / utils.sinkhorn / autograd.sinkhorn_divergence /
applications.sinkhorn_loss_fn / solvers.evaluate_ot_reference, against the float64 restatement of the same recursion on
the same schedule (tests/sinkhorn_ref.py), with the torch float32 composition of that recursion on the device -- direct
differences, logsumexp and softmax over materialised pair matrices -- as the yardstick for the fused error:
  e_fused <= 2 e_composed + floor.
The floors come from the float32 rounding of the argument's numerator h_j - C_ij, which is what either float32 route
exponentiates: potentials and S  8 * 2^-24 * (C_max + max|h|);  map and N xgrad  that figure times max_i sigma_i / eps,
sigma_i the standard deviation of row i of the x-y plan (a relative error r of the weights moves the barycentre by at
most r sigma_i, and an absolute error d of the numerator is a relative error d / eps of a weight).  C_max, max|h| and
sigma_i are the restatement's.  The schedules are geometric (ratio 0.5, 3 entries at eps: 10-20 iterations); no test
depends on the recursion having converged.

The kernel's own boundaries, each with a shape below, at and above it (BOUNDARY_SHAPES): 512 rows per workgroup (N = 511,
512, 513), 64 columns per tile (M = 63, 64, 65), the chunk of 4 columns (D <= 6; 2 beyond) inside a tile (M = 63, 65, 66,
67: tails of 3, 1, 2, 3 columns, and an odd count at D = 7), and the column split, which exceeds 1 from the first shape
whose longer side leaves one tile: max(N, M) = 65 (the split count is cnf_sinkhorn_splits, asserted below).

Measured on one MI355X (every test prints its figures: run with -s), errors against the restatement, fused / composed:
  the 33 sets of the parity cases   potentials 2.4e-8 .. 4.2e-6 / 3.9e-8 .. 8.7e-5, S 1.1e-10 .. 9.1e-8 / 8.2e-11 .. 1.4e-7,
                                    map 1.1e-8 .. 7.1e-5 / 1.1e-8 .. 1.6e-4, N xgrad 3.8e-8 .. 7.1e-5 / 2.9e-8 .. 1.6e-4
                                    (floors 1.5e-7 .. 1.7e-2: at most 0.25 of the floor, 0.15 of the bound)
  D=2 N=257 M=130 eps=0.01          potentials 3.6e-7 / 1.4e-5 (floor 2.7e-5), map 5.1e-6 / 1.6e-5 (floor 2.4e-3)
  D=10 N=300 M=257 eps=0.01         potentials 3.4e-6 / 8.6e-5 (floor 5.3e-5), map 7.1e-5 / 1.6e-4 (floor 1.7e-2)
  D=2 N=2048 M=1500 eps=0.05        potentials 2.3e-7 / 5.8e-6, S 2.8e-10 / 8.2e-11, N xgrad 5.0e-7 / 2.7e-6
  translation, 68 iterations        S within 1.6e-9 of |c|^2 / 2, N xgrad within 9.4e-5 of -c; S(x, x) = 0 exactly
  sinkhorn_loss_fn, D = 2 / 3       loss 3.8e-7 / 2.6e-7; parameter gradient 5.7e-7 / 7.9e-7 against flow_adjoint_f64.bound
                                    = 3.6e-5 / 1.1e-5; autograd.sinkhorn_divergence(flow_forward(...)) gave the fast
                                    path's gradient bit for bit
  evaluate_ot_reference, n = 1 024  w2_problem 9.472 against the closed form 9.930 (Gaussian source, 4.6 %), floor 1.9e-2,
                                    gap_flow 7.0e-2 (random parameters)
More cases: profiles/sinkhorn/README.md.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sinkhorn_ref as sr

ULP8 = 8.0 * 2.0 ** -24
ISSUE_SHAPES = [(1, 2, 2), (2, 65, 63), (2, 257, 130), (3, 64, 64), (10, 300, 257), (14, 129, 64), (2, 2048, 1500)]
# (D, N, M): rows per workgroup 512, columns per tile 64, columns per chunk 4 (2 from D = 7), the split count 1 -> 2
BOUNDARY_SHAPES = [(2, 511, 63), (2, 512, 64), (2, 513, 65), (3, 64, 2), (3, 65, 2), (7, 66, 67), (2, 1025, 1024)]
CASES = [(s, e) for s in ISSUE_SHAPES + BOUNDARY_SHAPES for e in (0.5, 0.05)] + [((2, 257, 130), 0.01), ((10, 300, 257), 0.01)]
_REF = {}


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def _inputs(D, N, M, index, S=None):
  return sr.clouds(D, N, M, seed=2000 + index, shift=0.2 + 0.1 * (index % 4), scale=1.0 + 0.125 * (index % 5), S=S)


def _ref(key, x, y, sched):
  """The restatement of one set, computed once per key and never changed"""
  if key not in _REF:
    _REF[key] = sr.run(x, y, sched)
  return _REF[key]


def _call(dev, x, y, sched, pot=True, grad=True, tmap=True, fill=None, stream=None, out=None):
  """cnf_sinkhorn through the C ABI on device tensors x [S, N, D], y [S, M, D]: a dict of sums [S, 6], pot
  [S, 2 N + 2 M], grad and map [S, N, D] (None where not asked for)"""
  from cnf_ot_amd import _capi
  from cnf_ot_amd.flows import _stream_ptr
  S, N, D = x.shape
  M = y.shape[1]
  lib = _capi.lib()
  nbytes = ctypes.c_int64(0)
  _capi.check(lib.cnf_sinkhorn_workspace(S, N, M, D, ctypes.byref(nbytes)), "cnf_sinkhorn_workspace")
  if out is None:
    out = {"ws": torch.zeros(nbytes.value, dtype=torch.uint8, device=dev),
           "sums": torch.full((S, 6), 7.25, dtype=torch.float64, device=dev),
           "pot": torch.full((S, 2 * (N + M)), 7.25, dtype=torch.float32, device=dev) if pot else None,
           "grad": torch.full((S, N, D), 7.25, dtype=torch.float32, device=dev) if grad else None,
           "map": torch.full((S, N, D), 7.25, dtype=torch.float32, device=dev) if tmap else None}
  if fill is not None:
    out["ws"].fill_(fill)
  assert x.is_contiguous() and y.is_contiguous() and x.dtype == torch.float32 and y.dtype == torch.float32
  ptr = lambda t: None if t is None else t.data_ptr()
  eps = (ctypes.c_double * len(sched))(*sched)
  _capi.check(lib.cnf_sinkhorn(S, x.data_ptr(), N, y.data_ptr(), M, D, eps, len(sched), out["sums"].data_ptr(),
                               ptr(out["pot"]), ptr(out["grad"]), ptr(out["map"]), out["ws"].data_ptr(), nbytes.value,
                               _stream_ptr(dev) if stream is None else stream), "cnf_sinkhorn")
  if stream is None:
    torch.cuda.synchronize()
  return out


def _composed(x, y, sched):
  """The same recursion as a torch float32 composition on the device: (potentials [2 N + 2 M], divergence, map [N, D],
  N xgrad [N, D]) as float64 numpy"""
  N, M = len(x), len(y)

  def arg(h, rows, cols, eps):
    diff = rows[:, None, :] - cols[None, :, :]
    return (h[None, :] - 0.5 * (diff * diff).sum(-1)) / np.float32(eps)

  def T(h, rows, cols, eps):
    return -np.float32(eps) * (torch.logsumexp(arg(h, rows, cols, eps), 1) - np.float32(np.log(len(cols))))

  f, g, p, q = (torch.zeros(n, dtype=torch.float32, device=x.device) for n in (N, M, N, M))
  for e in sched:
    f, g, p, q = 0.5 * (f + T(g, x, y, e)), 0.5 * (g + T(f, y, x, e)), 0.5 * (p + T(p, x, x, e)), 0.5 * (q + T(q, y, y, e))
  e = sched[-1]
  fs, gs, ps, qs = T(g, x, y, e), T(f, y, x, e), T(p, x, x, e), T(q, y, y, e)
  txy = torch.softmax(arg(g, x, y, e), 1) @ y
  txx = torch.softmax(arg(p, x, x, e), 1) @ x
  div = (fs.double().sum() - ps.double().sum()) / N + (gs.double().sum() - qs.double().sum()) / M
  return (torch.cat([fs, gs, ps, qs]).double().cpu().numpy(), float(div), txy.double().cpu().numpy(),
          (txx.double() - txy.double()).cpu().numpy())


def _div(sums, N, M):
  s = sums.cpu().numpy()
  return (s[0] - s[2]) / N + (s[1] - s[3]) / M


def _check(dev, x, y, sched, tag, key, got=None):
  """One set against the restatement under the bounds above; got: its slice of a call made elsewhere"""
  N, M = len(x), len(y)
  xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
  if got is None:
    o = _call(dev, xd[None], yd[None], sched)
    got = {k: o[k][0] for k in ("sums", "pot", "grad", "map")}
  r = _ref(key, x, y, sched)
  ref_pot = np.concatenate([r["f"], r["g"], r["p"], r["q"]])
  c_pot, c_div, c_map, c_g = _composed(xd, yd, sched)
  g_pot = got["pot"].double().cpu().numpy()
  g_div, g_map, g_g = _div(got["sums"], N, M), got["map"].double().cpu().numpy(), got["grad"].double().cpu().numpy() * N
  floor = ULP8 * (r["c_max"] + r["h_max"])
  floor_m = floor * float(r["sigma"].max()) / sched[-1]
  rows = [("potentials", np.abs(g_pot - ref_pot).max(), np.abs(c_pot - ref_pot).max(), floor),
          ("S", abs(g_div - r["divergence"]), abs(c_div - r["divergence"]), floor),
          ("map", np.abs(g_map - r["map"]).max(), np.abs(c_map - r["map"]).max(), floor_m),
          ("N xgrad", np.abs(g_g - r["xgrad"] * N).max(), np.abs(c_g - r["xgrad"] * N).max(), floor_m)]
  print(f"\n[sinkhorn {tag}] {len(sched)} iterations, S = {r['divergence']:.6f}, change {r['sums'][4]:.1e}: "
        + " | ".join(f"{n} fused {a:.2e} composed {b:.2e} floor {c:.2e}" for n, a, b, c in rows))
  assert np.isfinite(g_pot).all() and np.isfinite(g_map).all() and np.isfinite(g_g).all()
  # the sums are the potentials' own, and the diagnostic is the restatement's
  assert abs(float(got["sums"][0]) - g_pot[:N].sum()) <= 1e-12 * N * (1.0 + np.abs(g_pot).max())
  # (a change is the difference of two potentials, each allowed the potentials' bound)
  assert np.abs(got["sums"][4:].cpu().numpy() - r["sums"][4:]).max() <= 2.0 * (2.0 * rows[0][2] + floor)
  for name, a, b, c in rows:
    assert a <= 2.0 * b + c, (tag, name, a, b, c)


@pytest.mark.parametrize("shape,eps", CASES, ids=lambda v: "D%d-N%d-M%d" % v if isinstance(v, tuple) else f"eps{v}")
def test_parity_with_the_restatement(dev, shape, eps):
  D, N, M = shape
  index = (ISSUE_SHAPES + BOUNDARY_SHAPES).index(shape)
  x, y = _inputs(D, N, M, index)
  _check(dev, x, y, sr.schedule(x, y, eps, 0.5, 3), f"D={D} N={N} M={M} eps={eps}", ("parity", shape, eps))


def test_the_boundaries_named_above_are_the_kernels(dev):
  from cnf_ot_amd import _capi
  lib = _capi.lib()
  assert lib.cnf_sinkhorn_splits(1, 64, 2, 3) == 1 and lib.cnf_sinkhorn_splits(1, 65, 2, 3) == 2
  assert lib.cnf_sinkhorn_splits(1, 2, 2, 1) == 1 and lib.cnf_sinkhorn_splits(1, 65, 63, 2) == 2
  assert lib.cnf_sinkhorn_splits(1, 512, 64, 2) == 8 and lib.cnf_sinkhorn_splits(1, 513, 65, 2) == 9
  assert lib.cnf_sinkhorn_splits(1, 2048, 1500, 2) == 32 and lib.cnf_sinkhorn_splits(3, 257, 130, 2) == 5
  src = open(os.path.join(os.path.dirname(_capi.__file__), "csrc", "cnf_sinkhorn.hip")).read()
  assert "SK_THREADS = 256;" in src and "SK_R = 2;" in src and "SK_TILE = 64;" in src and "return D <= 6 ? 4 : 2;" in src


def test_three_sets_with_their_own_data(dev):
  D, N, M, S = 2, 257, 130, 3
  x, y = _inputs(D, N, M, 40, S=S)
  y[1] += 0.25                                           # (the sets differ in law as well as in draw)
  sched = sr.schedule(x, y, 0.05, 0.5, 3)                # one schedule: the box of all sets
  o = _call(dev, torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), sched)
  for s in range(S):
    _check(dev, x[s], y[s], sched, f"S=3 set {s}", ("sets", s), got={k: o[k][s] for k in ("sums", "pot", "grad", "map")})
  vals = [_div(o["sums"][s], N, M) for s in range(S)]
  assert len({round(v, 5) for v in vals}) == S           # three different numbers: no set read twice


def test_known_answers_through_the_python_surface(dev):
  from cnf_ot_amd import utils
  # translation: S = |c|^2 / 2 and N xgrad = -c for any eps at convergence (the CPU file's bars, widened by the floors)
  D, N, c = 2, 512, np.array([1.5, -0.75], dtype=np.float32)
  x, _ = sr.clouds(D, N, 2, seed=4)
  y = x + c
  c64 = (y.astype(np.float64) - x.astype(np.float64)).mean(0)      # (the shift as float32 made it)
  sched = sr.schedule(x, y, 0.5, 0.5, 60)
  r = _ref(("translation",), x, y, sched)
  res = utils.sinkhorn(x, y, schedule=sched, want_grad=True, want_map=True, want_potentials=True)
  assert set(res) == {"divergence", "ot_xy", "change", "grad", "map", "f", "g", "p", "q", "schedule"}
  assert res["divergence"].shape == (1,) and res["divergence"].dtype == torch.float64 and res["change"].shape == (1, 2)
  assert res["grad"].shape == (N, D) and res["map"].shape == (N, D) and res["f"].shape == (1, N) and res["g"].shape == (1, N)
  assert res["schedule"] == sched
  floor = ULP8 * (r["c_max"] + r["h_max"])
  floor_m = floor * float(r["sigma"].max()) / sched[-1]
  e_v = abs(float(res["divergence"][0]) - 0.5 * c64 @ c64)
  e_g = float(np.abs(res["grad"].double().cpu().numpy() * N + c64).max())
  e_m = float(np.abs(res["map"].double().cpu().numpy() - r["map"]).max())
  print(f"\n[sinkhorn translation] {len(sched)} iterations: value error {e_v:.2e} (bar 1e-6 + {floor:.1e}), N xgrad + c {e_g:.2e} "
        f"(bar 1e-3 + {floor_m:.1e}), map against the restatement {e_m:.2e}, change {res['change'][0].tolist()}")
  assert e_v <= 1e-6 + floor and e_g <= 1e-3 + floor_m
  assert abs(float(res["ot_xy"][0]) - r["ot_xy"]) <= 2.0 * floor
  # a cloud against itself: the four problems are one, S = 0 and no gradient
  same = utils.sinkhorn(x, x.copy(), schedule=sched[:12], want_grad=True)
  print(f"[sinkhorn S(x, x)] value {float(same['divergence'][0]):.3e}, largest |N xgrad| {float(same['grad'].abs().max()) * N:.3e}")
  assert abs(float(same["divergence"][0])) <= floor and float(same["grad"].abs().max()) * N <= floor_m
  assert same["map"] is None and same["f"] is None and len(same["schedule"]) == 12
  # the default schedule: utils.sinkhorn_schedule at eps, the device tensors and float64 inputs accepted
  d = utils.sinkhorn(torch.from_numpy(x).to(dev).double(), torch.from_numpy(y).to(dev), eps=0.5)
  assert d["schedule"] == utils.sinkhorn_schedule(x, y, 0.5) == sr.schedule(x, y, 0.5)
  assert d["grad"] is None and np.isfinite(float(d["divergence"][0]))


def test_invariants(dev):
  D, N, M, S = 3, 700, 1100, 2
  x, y = _inputs(D, N, M, 41, S=S)
  sched = sr.schedule(x, y, 0.05, 0.5, 3)
  xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
  a = _call(dev, xd, yd, sched)
  b = _call(dev, xd, yd, sched)
  for k in ("sums", "pot", "grad", "map"):                # two calls: the same bits
    assert torch.equal(a[k], b[k]), k
  c = _call(dev, xd, yd, sched, fill=0xFF)                # (0xFF bytes: NaN wherever the workspace is not rewritten)
  for k in ("sums", "pot", "grad", "map"):
    assert torch.equal(a[k], c[k]), k
  for want in ((False, False, False), (True, False, False), (False, True, False), (False, False, True)):
    o = _call(dev, xd, yd, sched, *want)                  # the value does not depend on what else is asked for
    assert torch.equal(a["sums"], o["sums"]), want
    for k, w in zip(("pot", "grad", "map"), want):
      assert o[k] is None or torch.equal(a[k], o[k]), (want, k)
  assert torch.isfinite(a["sums"]).all() and not bool((a["sums"] == 7.25).any())
  # views at an offset that is 4-byte but not 16-byte aligned
  bx = torch.zeros(x.size + 1, dtype=torch.float32, device=dev)
  by = torch.zeros(y.size + 3, dtype=torch.float32, device=dev)
  xv, yv = bx[1:].view(S, N, D), by[3:].view(S, M, D)
  xv.copy_(xd)
  yv.copy_(yd)
  assert xv.data_ptr() % 16 == 4 and yv.data_ptr() % 16 == 12
  o = _call(dev, xv, yv, sched)
  assert torch.equal(a["sums"], o["sums"]) and torch.equal(a["grad"], o["grad"])


def test_a_nan_coordinate_stays_in_its_set(dev):
  D, N, M, S = 2, 257, 130, 3
  x, y = _inputs(D, N, M, 42, S=S)
  sched = sr.schedule(x, y, 0.05, 0.5, 3)
  xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
  clean = _call(dev, xd, yd, sched)
  xd[1, 100, 1] = float("nan")
  o = _call(dev, xd, yd, sched)                           # (the call returns: every loop of the kernels is counted)
  assert torch.equal(o["sums"][0], clean["sums"][0]) and torch.equal(o["sums"][2], clean["sums"][2])
  assert torch.equal(o["grad"][0], clean["grad"][0]) and torch.equal(o["pot"][2], clean["pot"][2])
  # x is a row of f and p and a column of g: the three turn NaN, and with them the divergence; q never sees x
  s1 = o["sums"][1]
  assert bool(torch.isnan(s1[:3]).all()) and bool(torch.isnan(s1[4:]).all()) and bool(torch.isfinite(s1[3]))
  assert np.isnan(_div(s1, N, M))


def test_a_captured_call_replays_the_eager_bits(dev):
  D, N, M, S = 2, 300, 257, 2
  x, y = _inputs(D, N, M, 43, S=S)
  sched = sr.schedule(x, y, 0.05, 0.5, 3)[:12]
  assert len(sched) == 12
  xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
  eager = _call(dev, xd, yd, sched)
  replay = _call(dev, xd, yd, sched[:1])                  # buffers of the same shapes, holding another call's numbers
  torch.cuda.synchronize()
  side = torch.cuda.Stream(device=dev)
  side.wait_stream(torch.cuda.current_stream(dev))
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side):              # (the call's launches are one linear chain)
    _call(dev, xd, yd, sched, stream=side.cuda_stream, out=replay)
  for _ in range(2):
    for k in ("sums", "pot", "grad", "map"):
      replay[k].fill_(7.25)
    graph.replay()
    torch.cuda.synchronize()
    for k in ("sums", "pot", "grad", "map"):
      assert torch.isfinite(eager[k]).all() and torch.equal(eager[k], replay[k]), k


@pytest.mark.parametrize("D", [2, 3])
def test_training_term_against_the_float64_adjoint(dev, D):
  import sample_term_check
  from cnf_ot_amd import applications as app, autograd
  B, M = 256, 130
  _, tgt = _inputs(D, 2, M, 46 + D)
  sched = [16.0, 8.0, 4.0, 2.0, 1.0, 0.5, 0.25, 0.25, 0.25, 0.25]

  def restate(out):      # (the envelope gradient)
    r = sr.run(out, tgt, sched)
    return r["divergence"], r["xgrad"], r
  sample_term_check.check(dev, f"sinkhorn_loss_fn D={D}", D, B, tgt, app.sinkhorn_loss_fn, dict(schedule=sched),
                          auto=lambda x, y: autograd.sinkhorn_divergence(x, y, schedule=sched), restate=restate,
                          floor=lambda out64, runs: ULP8 * max(r["c_max"] + r["h_max"] for r in runs))


@pytest.mark.parametrize("source", ["mixture", "gaussian"])
def test_evaluate_ot_reference(dev, source):
  from cnf_ot_amd import FlowConfig, Params, solvers
  config = solvers.load_config(overrides={"general": {"type": "ot", "dim": 2}, "ot": {"source": source}})
  model = solvers.build_model(config)
  params = Params.random(FlowConfig(dim=2), 0.2, seed=4, device=dev)
  eps = 0.05
  res = solvers.evaluate_ot_reference(config, model, params, n=1024, eps=eps, seed=5)
  assert set(res) == set(solvers.OT_REFERENCE_KEYS)
  solvers.print_ot_reference(res)
  for k, v in res.items():
    if k == "w2_closed_form" and source == "mixture":
      assert v is None
    else:
      assert np.isfinite(np.asarray(v, dtype=np.float64)).all(), (k, v)
  assert np.asarray(res["change"]).shape == (5, 2) and res["n"] == 1024 and res["eps"] == eps
  # the flow's own coupling cannot cost less than the optimal one, up to the estimate's noise and entropic bias
  assert res["gap_flow"] >= -res["floor"] - 2.0 * eps
  assert res["gap_flow"] == res["coupling_cost"] - res["w2_flow"]
  if source == "gaussian":
    assert abs(res["w2_closed_form"] - 19.861 / 2.0) <= 1e-3
    print(f"[evaluate_ot_reference] w2_problem {res['w2_problem']:.4f} against the closed form {res['w2_closed_form']:.4f}")
    assert abs(res["w2_problem"] / res["w2_closed_form"] - 1.0) <= 0.05
