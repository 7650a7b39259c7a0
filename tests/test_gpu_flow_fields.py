"""The fused field kernel (cnf_eulerian_fields / cnf_trajectories, float32 and float64) through the C ABI wrappers of
FlowEngine and through cnf_ot_amd.utils / solvers.figure_data, against tests/flow_fields_f64.py.

Bounds (derived, not measured):
  float64: logp and traj take the bound test_float64_kernels_match_oracle_to_1e12 holds its golden vectors to,
    B64 = 1e-11 x max(1, |want|); vel and score are differences of two such values over dt / dx: B64 x 2 / dt and
    B64 x 2 / dx; rho = exp(logp): the logp bound relative to rho.
  float32: logp the existing 1e-5 (test_gpu_parity.TOL_LP_DATA_MAX, with its 2-ulp allowance _err), rho the same
    relative to rho; traj the existing TOL_Y = 2e-5; vel and score -- differences of two fp32 passes over 0.01 -- at
    most 2 x the maximum error of the oracle's own float32 instantiation on the same inputs (the criterion of the
    `wild` set), both printed.
"""
import ctypes

import numpy as np
import pytest
import torch

import flow_fields_f64 as ff
from network_shapes import networks, param_scale
from test_gpu_parity import RTOL, TOL_LP_DATA_MAX, TOL_Y, _err

pytestmark = pytest.mark.gpu

B64 = 1e-11
DT = DX = 0.01
T_ARRAY = np.array([0.0, 0.5, 1.0, 1.75])      # (exact in float32: both kernels and the oracle see the same times)
T0 = 0.25
DIMS = (2, 3, 10)


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "gpu tests need a ROCm device"
  return torch.device("cuda", 0)


def _cfgs(D, H=16, K=5, M=2, L=2):
  import oracle
  from cnf_ot_amd import FlowConfig
  # (the C ABI carries the spline constants as float32: the oracle gets the same rounded values)
  return (FlowConfig(dim=D, num_layers=L, hidden_size=H, mlp_num_layers=M, num_bins=K),
          oracle.OracleConfig(D=D, L=L, H=H, M=M, K=K, min_bin_size=float(np.float32(1e-4)),
                              min_knot_slope=float(np.float32(1e-4))))


def _setup(D, dev, H=16, K=5, M=2, L=2, seed=0):
  from cnf_ot_amd import FlowEngine, FlowModel, Params
  fcfg, ocfg = _cfgs(D, H, K, M, L)
  s = param_scale(H, M, D)
  flat = np.random.default_rng([H, K, M, L, D, seed]).normal(0.0, s, fcfg.param_count()).astype(np.float32)
  params = Params(fcfg, torch.from_numpy(flat).to(dev))
  model = FlowModel(fcfg)
  return model, params, model.engine(dev).load(params), ocfg, flat


def _points(D, n, seed):
  """inside |r| <= 5, where the float32 port itself is meaningful"""
  return np.random.default_rng(seed).uniform(-3.0, 3.0, (n, D)).astype(np.float32).astype(np.float64)


def _np(t):
  return t.detach().cpu().numpy().astype(np.float64)


def _want(flow, pts, r0):
  return {"logp": np.stack([flow.log_prob(pts.astype(flow.dtype), flow.dtype(t)) for t in T_ARRAY]).astype(np.float64),
          "vel": ff.velocity_field(flow, pts, T_ARRAY, DT).astype(np.float64),
          "score": ff.score_field(flow, pts, T_ARRAY, DX).astype(np.float64),
          "traj": ff.trajectories(flow, r0, T_ARRAY, T0).astype(np.float64),
          "tvel": ff.trajectory_velocity(flow, r0, T_ARRAY, T0, DT).astype(np.float64)}


def _got(eng, pts, r0, dtype):
  p = torch.from_numpy(pts).to(eng.device, dtype)
  res = eng.eulerian_fields(T_ARRAY, pts=p, rho=True, logp=True, vel=True, score=True, dt=DT, dx=DX)
  assert res is not None and eng.last_path() == ("f64" if dtype == torch.float64 else "fields")
  traj, tvel = eng.trajectories(torch.from_numpy(r0).to(eng.device, dtype), T_ARRAY, T0, vel=True, dt=DT)
  res.update(traj=traj, tvel=tvel)
  assert all(v.dtype == dtype for v in res.values())
  return {k: _np(v) for k, v in res.items()}


@pytest.mark.parametrize("D", DIMS)
def test_float64_kernels_match_the_oracle(oracle_lib, dev, D):
  model, params, eng, ocfg, flat = _setup(D, dev)
  pts, r0 = _points(D, 777, 1), _points(D, 300, 2)
  want = _want(ff.OracleFlow(ocfg, flat), pts, r0)
  got = _got(eng, pts, r0, torch.float64)
  one = lambda a: np.maximum(1.0, np.abs(a))
  pos = max(1.0, np.abs(want["traj"]).max(), np.abs(pts).max())
  errs = {
    "logp": (np.abs(got["logp"] - want["logp"]) / one(want["logp"])).max() / B64,
    "rho": (np.abs(got["rho"] - np.exp(want["logp"])) / (np.exp(want["logp"]) * one(want["logp"]))).max() / B64,
    "traj": (np.abs(got["traj"] - want["traj"]) / one(want["traj"])).max() / B64,
    "vel": np.abs(got["vel"] - want["vel"]).max() / (B64 * pos * 2 / DT),
    "tvel": np.abs(got["tvel"] - want["tvel"]).max() / (B64 * pos * 2 / DT),
    "score": np.abs(got["score"] - want["score"]).max() / (B64 * one(want["logp"]).max() * 2 / DX),
  }
  print(f"\n[fields f64 dim {D}] error / bound: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
  assert all(v <= 1.0 for v in errs.values()), errs


@pytest.mark.parametrize("D", DIMS)
def test_float32_kernels_match_the_oracle(oracle_lib, dev, D):
  model, params, eng, ocfg, flat = _setup(D, dev)
  pts, r0 = _points(D, 777, 1), _points(D, 300, 2)
  want = _want(ff.OracleFlow(ocfg, flat), pts, r0)
  port = _want(ff.OracleFlow(ocfg, flat, np.float32), pts, r0)
  got = _got(eng, pts, r0, torch.float32)
  e_lp = np.maximum(np.abs(got["logp"] - want["logp"]) - RTOL * np.abs(want["logp"]), 0.0).max()
  rho = np.exp(want["logp"])
  e_rho = (np.abs(got["rho"] - rho) / rho - RTOL * (1.0 + np.abs(want["logp"]))).max()
  e_traj = np.maximum(np.abs(got["traj"] - want["traj"]) - RTOL * np.abs(want["traj"]), 0.0).max()
  print(f"\n[fields f32 dim {D}] logp {e_lp:.2e} (bar {TOL_LP_DATA_MAX:.0e}) rho rel {e_rho:.2e} traj {e_traj:.2e} "
        f"(bar {TOL_Y:.0e})")
  ratios = {}
  for k in ("vel", "tvel", "score"):
    e_port, e_gpu = np.abs(port[k] - want[k]).max(), np.abs(got[k] - want[k]).max()
    ratios[k] = e_gpu / e_port
    print(f"[fields f32 dim {D}] {k}: port max error {e_port:.3e}, gpu max error {e_gpu:.3e}")
  assert e_lp <= TOL_LP_DATA_MAX and e_rho <= TOL_LP_DATA_MAX and e_traj <= TOL_Y
  assert all(r <= 2.0 for r in ratios.values()), ratios


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_fused_equals_composed(oracle_lib, dev, D, dtype):
  """utils.* with the fused kernel against the same fields composed from model.apply.log_prob / inverse / forward call
  by call: rho on a non-square grid slice, logp, vel and score at points, vel on the grid, traj and the velocity along
  it.

  float64: |fused - composed| within the derived bound of the module docstring, element by element (rho: the logp bound
  relative to rho).
  float32: with the composition forced onto the kernels the fused one is built from (scalar-weight conditioner, one
  sample per lane) traj and logp are bit for bit.  Everything else -- the composition under its default kernel choice
  (MFMA conditioner / wave-per-dimension kernel for launches this small), and vel / score on either path, where two
  float32 differences over 0.01 need not round alike -- takes the float32 bounds of the module docstring, EACH side
  against the float64 helper on the same inputs: logp 1e-5, rho 1e-5 relative, traj 2e-5 (with the 2-ulp allowance),
  vel / vel_grid / tvel / score at most 2 x the float32 port's maximum error.  This also holds the composed float32
  velocity and score (FlowEngine.logprob_fd) to the helper."""
  from cnf_ot_amd import utils
  model, params, eng, ocfg, flat = _setup(D, dev)
  pts64, r064 = _points(D, 500, 3), _points(D, 100, 4)
  pts = torch.from_numpy(pts64).to(dev, dtype)
  r0 = torch.from_numpy(r064).to(dev, dtype)
  g = utils.field_grid([-2.0, 2.0, -1.5, 1.5], (23, 17), axes=(0, D - 1), fixed=0.25)

  def fields(fused):
    out = {"rho": utils.density_on_grid(model, params, T_ARRAY, g["domain_range"], g["n"], g["axes"], 0.25, dtype=dtype,
                                        fused=fused).reshape(len(T_ARRAY), -1),
           "logp": utils.eulerian_fields(model, params, pts, T_ARRAY, logp=True, fused=fused)["logp"],
           "vel": utils.velocity_field(model, params, pts, T_ARRAY, DT, fused=fused),
           "vel_grid": utils.velocity_field(model, params, g, T_ARRAY, DT, dtype=dtype, fused=fused),
           "score": utils.score_field(model, params, pts, T_ARRAY, DX, fused=fused)}
    out["traj"], out["tvel"] = utils.trajectories(model, params, r0, T_ARRAY, T0, True, DT, fused=fused)
    return out

  a, b = fields(True), fields(False)
  assert a["rho"].shape == (len(T_ARRAY), 17 * 23) and a["vel_grid"].shape == (len(T_ARRAY), 17 * 23, D)
  assert all(v.dtype == dtype for v in list(a.values()) + list(b.values()))
  if dtype == torch.float64:
    d = {k: (a[k] - b[k]).abs() for k in a}
    one = lambda x: x.abs().clamp(min=1.0)
    pos = max(1.0, b["traj"].abs().max().item(), 3.0)
    lp = one(b["logp"]).max().item()
    errs = {"rho": (d["rho"] / (b["rho"] * one(torch.log(b["rho"])))).max().item() / B64,
            "logp": (d["logp"] / one(b["logp"])).max().item() / B64,
            "traj": (d["traj"] / one(b["traj"])).max().item() / B64,
            "vel": d["vel"].max().item() / (B64 * pos * 2 / DT),
            "vel_grid": d["vel_grid"].max().item() / (B64 * pos * 2 / DT),
            "tvel": d["tvel"].max().item() / (B64 * pos * 2 / DT),
            "score": d["score"].max().item() / (B64 * lp * 2 / DX)}
    print(f"\n[fused vs composed f64 dim {D}] difference / bound: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= 1.0 for v in errs.values()), errs
    return
  # the composition on the same kernel path
  eng.set_mfma(0); eng.set_dpar(0); eng.set_samples_per_lane(1)
  try:
    c = fields(False)
    assert eng.last_path() == "mlp1"
  finally:
    eng.set_mfma(2); eng.set_dpar(1); eng.set_samples_per_lane(0)
  # the float64 helper and the float32 port on the inputs the kernels see: the float32 grid points
  XY = utils.field_grid_points(g, D).astype(np.float32).astype(np.float64)
  f64, f32 = ff.OracleFlow(ocfg, flat), ff.OracleFlow(ocfg, flat, np.float32)
  want, port = _want(f64, pts64, r064), _want(f32, pts64, r064)
  want["vel_grid"] = ff.velocity_field(f64, XY, T_ARRAY, DT).astype(np.float64)
  port["vel_grid"] = ff.velocity_field(f32, XY, T_ARRAY, DT).astype(np.float64)
  lp_grid = np.stack([f64.log_prob(XY, t) for t in T_ARRAY])
  fails = []
  for side, got in (("fused", a), ("composed", b), ("composed, same kernels", c)):
    got = {k: _np(v) for k, v in got.items()}
    e_lp = np.maximum(np.abs(got["logp"] - want["logp"]) - RTOL * np.abs(want["logp"]), 0.0).max()
    e_rho = (np.abs(got["rho"] - np.exp(lp_grid)) / np.exp(lp_grid) - RTOL * (1.0 + np.abs(lp_grid))).max()
    e_traj = np.maximum(np.abs(got["traj"] - want["traj"]) - RTOL * np.abs(want["traj"]), 0.0).max()
    print(f"\n[{side} f32 dim {D}] logp {e_lp:.2e} (bar {TOL_LP_DATA_MAX:.0e}) rho rel {e_rho:.2e} traj {e_traj:.2e} "
          f"(bar {TOL_Y:.0e})")
    if not (e_lp <= TOL_LP_DATA_MAX and e_rho <= TOL_LP_DATA_MAX and e_traj <= TOL_Y):
      fails.append((side, e_lp, e_rho, e_traj))
    for k in ("vel", "vel_grid", "tvel", "score"):
      e_port, e_gpu = np.abs(port[k] - want[k]).max(), np.abs(got[k] - want[k]).max()
      print(f"[{side} f32 dim {D}] {k}: port max error {e_port:.3e}, gpu max error {e_gpu:.3e}")
      if not e_gpu <= 2.0 * e_port:
        fails.append((side, k, e_gpu, e_port))
  assert not fails, fails
  assert torch.equal(a["traj"], c["traj"])
  assert torch.equal(a["logp"], c["logp"])


def test_projected_density_three_directions(oracle_lib, dev):
  """dim 3, 11 sections, each direction of plot_proj_density; two calls bit-identical (fixed summation order)."""
  from cnf_ot_amd import solvers, utils
  model, params, eng, ocfg, flat = _setup(3, dev)
  st = solvers.FIGURE_SETTINGS[("fp", "lorenz", 3)]
  sec = np.linspace(-5.0, 5.0, 11)
  dom, n, ts = st["domain_range"], (40, 30), T_ARRAY[:2]
  flow = ff.OracleFlow(ocfg, flat)
  for name, (axes, sec_axis) in st["directions"].items():
    want = ff.density_on_grid(flow, ts, dom, n, axes, None, sec, sec_axis)
    # per section: log_prob on the grid, for the bound of the mean -- every term within its own relative bound
    lps = np.stack([ff.log_density_on_grid(flow, ts, dom, n, axes, [v if d == sec_axis else 0.0 for d in range(3)])
                    for v in sec])
    for dtype in (torch.float64, torch.float32):
      got = utils.density_on_grid(model, params, ts, dom, n, axes, section=sec, section_axis=sec_axis, dtype=dtype)
      assert eng.last_path() == ("f64" if dtype == torch.float64 else "fields")
      again = utils.density_on_grid(model, params, ts, dom, n, axes, section=sec, section_axis=sec_axis, dtype=dtype)
      assert torch.equal(got, again)
      assert got.shape == (2, 30, 40)
      eps = B64 * np.maximum(1.0, np.abs(lps)) if dtype == torch.float64 else TOL_LP_DATA_MAX + RTOL * (1.0 + np.abs(lps))
      bar = (np.exp(lps) * eps).mean(0) + (0.0 if dtype == torch.float64 else RTOL * want)
      ratio = (np.abs(_np(got) - want) / bar).max()
      print(f"\n[proj {name} {dtype}] max error / bound {ratio:.2e}")
      assert ratio <= 1.0


@pytest.mark.parametrize("net", networks(), ids=lambda n: n.id)
def test_every_network_density_at_dim_2(oracle_lib, dev, net):
  from cnf_ot_amd import utils
  model, params, eng, ocfg, flat = _setup(2, dev, net.H, net.K, net.M, net.L)
  dom, n = [-3.0, 3.0, -2.5, 2.5], (24, 20)
  lp = ff.log_density_on_grid(ff.OracleFlow(ocfg, flat), T_ARRAY, dom, n)
  for dtype in (torch.float64, torch.float32):
    got = _np(utils.density_on_grid(model, params, T_ARRAY, dom, n, dtype=dtype))
    assert eng.last_path() == ("f64" if dtype == torch.float64 else "fields")
    rel = np.abs(got - np.exp(lp)) / np.exp(lp)
    if dtype == torch.float64:
      assert (rel / np.maximum(1.0, np.abs(lp))).max() <= B64, (net.id, rel.max())
    else:
      assert (rel - RTOL * (1.0 + np.abs(lp))).max() <= TOL_LP_DATA_MAX, (net.id, rel.max())


@pytest.mark.parametrize("case", ["dim17", "periodized"])
def test_unsupported_configurations_are_composed(dev, case):
  from cnf_ot_amd import FlowConfig, FlowModel, Params, _capi, utils
  cfg = FlowConfig(dim=17) if case == "dim17" else FlowConfig.torus(dim=2)
  D = cfg.dim
  model = FlowModel(cfg)
  params = Params.random(cfg, 0.05, seed=3, device=dev)
  eng = model.engine(dev).load(params)
  lo, hi = (-2.0, 2.0) if case == "dim17" else (0.5, 5.5)
  pts = torch.from_numpy(np.random.default_rng(1).uniform(lo, hi, (300, D)).astype(np.float32)).to(dev)
  t = torch.tensor(T_ARRAY, dtype=torch.float32, device=dev)
  out = torch.empty(len(T_ARRAY), 300, device=dev)
  for dtype, fn, tr in ((torch.float32, eng.lib.cnf_eulerian_fields, eng.lib.cnf_trajectories),
                        (torch.float64, eng.lib.cnf_eulerian_fields_f64, eng.lib.cnf_trajectories_f64)):
    p, tt, o = pts.to(dtype), t.to(dtype), out.to(dtype)
    o3 = torch.empty(len(T_ARRAY), 300, D, dtype=dtype, device=dev)
    rc = fn(eng._h, None, p.data_ptr(), 300, tt.data_ptr(), len(T_ARRAY), DT, DX, None, o.data_ptr(), None, None, None)
    assert rc == _capi.CNF_ERR_UNSUPPORTED
    rc = tr(eng._h, p.data_ptr(), 300, 0.0, tt.data_ptr(), len(T_ARRAY), DT, o3.data_ptr(), None, None)
    assert rc == _capi.CNF_ERR_UNSUPPORTED
  assert eng.eulerian_fields(T_ARRAY, pts=pts, logp=True) is None and eng.trajectories(pts, T_ARRAY) is None
  dom = [lo, hi, lo, hi]
  rho = utils.density_on_grid(model, params, T_ARRAY, dom, (9, 7), fixed=1.0)
  XY = torch.from_numpy(utils.field_grid_points(utils.field_grid(dom, (9, 7), fixed=1.0), D)).to(dev, torch.float32)
  for j, tj in enumerate(T_ARRAY):
    lp = model.apply.log_prob(params, XY, cond=float(np.float32(tj)))
    assert torch.equal(rho[j].reshape(-1), torch.exp(lp.double()).float())
  traj = utils.trajectories(model, params, pts, T_ARRAY, 0.0)
  xi = model.apply.inverse(params, pts, 0.0)
  assert torch.equal(traj[2], model.apply.forward(params, xi, float(np.float32(T_ARRAY[2]))))
  vel = utils.velocity_field(model, params, pts, T_ARRAY)
  score = utils.score_field(model, params, pts, T_ARRAY)
  assert vel.shape == score.shape == (len(T_ARRAY), 300, D)
  assert torch.isfinite(vel).all() and torch.isfinite(score).all() and torch.isfinite(rho).all()


def test_empty_calls_answer_like_full_ones(dev):
  """N = 0 or S = 0: CNF_OK without a launch on a model the kernel serves, CNF_ERR_UNSUPPORTED on one it does not --
  the answer a call with points gives -- and an unsupported call leaves last_path alone."""
  from cnf_ot_amd import FlowConfig, FlowModel, Params, _capi
  t = torch.tensor(T_ARRAY, dtype=torch.float32, device=dev)
  for cfg, want in ((FlowConfig(dim=3), _capi.CNF_OK), (FlowConfig(dim=17), _capi.CNF_ERR_UNSUPPORTED)):
    eng = FlowModel(cfg).engine(dev).load(Params.random(cfg, 0.05, seed=3, device=dev))
    pts = torch.zeros(4, cfg.dim, device=dev)
    eng.log_prob(pts, torch.tensor([0.5], device=dev))
    path = eng.last_path()
    out = torch.empty(len(T_ARRAY), 4, cfg.dim, device=dev)
    for N, S in ((0, len(T_ARRAY)), (4, 0), (0, 0)):
      assert eng.lib.cnf_eulerian_fields(eng._h, None, pts.data_ptr(), N, t.data_ptr(), S, DT, DX, None, out.data_ptr(),
                                         None, None, None) == want
      assert eng.lib.cnf_trajectories(eng._h, pts.data_ptr(), N, 0.0, t.data_ptr(), S, DT, out.data_ptr(), None,
                                      None) == want
    if want != _capi.CNF_OK:
      assert eng.lib.cnf_trajectories(eng._h, pts.data_ptr(), 4, 0.0, t.data_ptr(), len(T_ARRAY), DT, out.data_ptr(),
                                      None, None) == want
    assert eng.last_path() == path


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_non_finite_points_come_out_non_finite(dev, dtype):
  model, params, eng, ocfg, flat = _setup(3, dev)
  pts = torch.from_numpy(_points(3, 600, 7)).to(dev, dtype)
  kw = dict(rho=True, logp=True, vel=True, score=True, dt=DT, dx=DX)
  clean = eng.eulerian_fields(T_ARRAY, pts=pts, **kw)
  bad = pts.clone()
  bad[5, 0] = float("nan")
  bad[300, 2] = float("inf")
  bad[599, 1] = float("-inf")
  res = eng.eulerian_fields(T_ARRAY, pts=bad, **kw)
  rows = torch.tensor([5, 300, 599], device=dev)
  keep = torch.ones(600, dtype=torch.bool, device=dev)
  keep[rows] = False
  for k in ("rho", "logp", "vel", "score"):
    assert torch.isnan(res[k][:, rows]).all(), k
    assert torch.equal(res[k][:, keep], clean[k][:, keep]), k
  traj, tvel = eng.trajectories(bad, T_ARRAY, T0, vel=True)
  ctraj, ctvel = eng.trajectories(pts, T_ARRAY, T0, vel=True)
  assert torch.isnan(traj[:, rows]).all() and torch.isnan(tvel[:, rows]).all()
  assert torch.equal(traj[:, keep], ctraj[:, keep]) and torch.equal(tvel[:, keep], ctvel[:, keep])


def test_calls_replay_from_a_graph_bit_for_bit_and_never_allocate(dev):
  """The check of test_compute_calls_never_allocate: the C calls captured into a graph on a single side stream (an
  allocation or a synchronisation would fail the capture); the replay equals the eager call."""
  from cnf_ot_amd import _capi
  model, params, eng, ocfg, flat = _setup(3, dev)
  S, nx, ny, D = len(T_ARRAY), 37, 29, 3
  N = nx * ny
  t = torch.tensor(T_ARRAY, dtype=torch.float32, device=dev)
  fixed = torch.tensor([0.0, 0.0, 3.0], device=dev)
  sec = torch.tensor([3.0], device=dev)
  g = _capi.CnfFieldGrid(-2.0, -2.0, 4.0 / (nx - 1), 4.0 / (ny - 1), nx, ny, 0, 1, 2, 1, fixed.data_ptr(), sec.data_ptr())
  r0 = torch.from_numpy(_points(D, 333, 8)).to(dev, torch.float32)
  mk = lambda *shape: torch.full(shape, -7.0, device=dev)

  def run(out, stream):
    rho, logp, vel, score, traj, tvel = out
    _capi.check(eng.lib.cnf_eulerian_fields(eng._h, ctypes.byref(g), None, N, t.data_ptr(), S, DT, DX, rho.data_ptr(),
                                            logp.data_ptr(), vel.data_ptr(), score.data_ptr(), stream), "fields")
    _capi.check(eng.lib.cnf_trajectories(eng._h, r0.data_ptr(), 333, T0, t.data_ptr(), S, DT, traj.data_ptr(),
                                         tvel.data_ptr(), stream), "trajectories")

  new = lambda: (mk(S, N), mk(S, N), mk(S, N, D), mk(S, N, D), mk(S, 333, D), mk(S, 333, D))
  eager, replay = new(), new()
  run(eager, torch.cuda.current_stream(dev).cuda_stream)
  torch.cuda.synchronize()
  side = torch.cuda.Stream(device=dev)
  side.wait_stream(torch.cuda.current_stream(dev))
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side):
    run(replay, side.cuda_stream)
  graph.replay()
  torch.cuda.synchronize()
  for a, b in zip(eager, replay):
    assert torch.isfinite(a).all() and torch.equal(a, b)
  # the grid generated in the kernel is the reference's XY, the section value its third column
  XY = torch.from_numpy(ff.grid_points([-2.0, 2.0, -2.0, 2.0], (nx, ny), 3, fixed=[0.0, 0.0, 3.0])).to(dev, torch.float32)
  want = eng.eulerian_fields(T_ARRAY, pts=XY, logp=True)["logp"]
  assert torch.equal(eager[1], want)


@pytest.mark.parametrize("trained", [False, True], ids=["identity", "trained"])
def test_figure_data_on_the_default_config(dev, trained):
  from cnf_ot_amd import solvers
  config = solvers.load_config()
  if trained:
    model, params, _ = solvers.train(config, epochs=30)
  else:
    model = solvers.build_model(config)
    params = model.init(config["general"]["seed"])
  fd = solvers.figure_data(config, model, params)
  assert set(fd) == {"t_array", "r0", "domain_range", "density", "trajectories"}
  assert fd["density"].shape == (5, 100, 100) and fd["trajectories"].shape == (5, 8, 2)
  assert all(torch.isfinite(v).all() for v in fd.values())
  x = np.linspace(-2.0, 2.0, 100)
  X, Y = np.meshgrid(x, x)
  XY = torch.from_numpy(np.hstack([X.reshape(-1, 1), Y.reshape(-1, 1)])).to(dev, torch.float32)      # utils.py:615-618
  for j, t in enumerate(np.linspace(0.0, 2.0, 5)):
    lp = model.apply.log_prob(params, XY, cond=float(t)).double()
    rho = torch.exp(lp).reshape(100, 100)
    rel = ((fd["density"][j].double() - rho).abs() / rho).max().item()
    assert rel <= 2 * (TOL_LP_DATA_MAX + RTOL * (1.0 + lp.abs().max().item())), (j, rel)
  assert (fd["trajectories"][0] - fd["r0"]).abs().max().item() <= 2 * TOL_Y        # t_array[0] = t0 = 0
  if not trained:
    assert (fd["trajectories"] - fd["r0"][None]).abs().max().item() <= 2 * TOL_Y    # the identity flow moves nothing


def test_new_entry_points_are_exported_and_bound():
  from cnf_ot_amd import _capi
  lib = _capi.lib()
  import os
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  with open(os.path.join(root, "include", "cnf_ot_amd.h")) as f:
    header = f.read()
  for name in ("cnf_eulerian_fields", "cnf_eulerian_fields_f64", "cnf_trajectories", "cnf_trajectories_f64"):
    assert name in _capi.SYMBOLS and hasattr(lib, name) and f"int {name}(" in header, name
    assert getattr(lib, name).argtypes == _capi.SYMBOLS[name][1]
  assert ctypes.sizeof(_capi.CnfFieldGrid) == 4 * 8 + 6 * 4 + 2 * 8
