"""GPU tests of cnf_fp_particles / cnf_point_stats, the Euler-Maruyama particle reference of the fp problems: the paths
against the float64 restatement (tests/fp_particles_f64.py) fed the device's own normals, the sums and the histogram
against NumPy on the kernel's own positions, a split ensemble, repeated calls, a non-finite start, the
Ornstein-Uhlenbeck statistics of test_fp_particles_cpu on the device, and solvers.evaluate_fp_path against its
composition.

Path tolerance.  Kernel and restatement are both float64 and differ in operation order and FMA contraction only, so what
must be bounded is how the dynamics amplify a last-bit difference.  That is measured, not assumed: per drift and
snapshot, the restatement's own divergence when every start coordinate moves by one ulp, times 64, with the floor
1e-13 max(1, |x|).  Measured (N = 1000, h = 0.01, divergence at steps 0 / 1 / 18 / 37, maximum over the ensemble):
  ou D = 1               8.9e-16 at every step
  ou D = 2, 5, nongradient  4.4e-16 -> 8.9e-16
  gradient               4.4e-16 / 4.4e-16 / 1.0e-15 / 1.7e-15
  lorenz                 4.4e-16 / 8.9e-16 / 1.0e-14 / 4.1e-14   (max |x| 3.6 -> 8.7)
so the bound is the floor (1e-13 to 5e-13) everywhere but Lorenz at step 37, 2.6e-12.  The test measures them again on
the normals it uses and prints them next to the kernel's error.
"""
import math

import numpy as np
import pytest
import torch

import fp_particles_f64 as fp
OU, OU_SEED, ou_check = fp.OU, fp.OU_SEED, fp.ou_check

pytestmark = pytest.mark.gpu
CASES = [("ou", 1), ("ou", 2), ("ou", 5), ("gradient", 2), ("nongradient", 2), ("lorenz", 3)]
N, H, STEPS, SNAPS = 1000, 0.01, 37, (0, 1, 18, 37)          # 1000: no multiple of the chunk of 256
A, SIGMA, VAR0, SEED = 1.0, 0.5, 1.0, 11
GRID = dict(lo=(-1.5, -1.0), step=(0.5, 0.5), n=(7, 5), axes=(0, 1))      # leaves particles outside on every side


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda", 0)


def _c_grid(g, axes=None):
  from cnf_ot_amd import _capi
  ax = g["axes"] if axes is None else axes
  return _capi.CnfFieldGrid(g["lo"][0], g["lo"][1], g["step"][0], g["step"][1], g["n"][0], g["n"][1], ax[0], ax[1], -1, 1,
                            None, None)


def run(dev, subtype, D, n=N, first=0, x0=None, grid=GRID, snaps=SNAPS, steps=STEPS, seed=SEED, sigma=SIGMA):
  """One cnf_fp_particles call with every output (the histogram where the event has two axes): numpy pos, sums, hist"""
  from cnf_ot_amd import _capi
  lib, C = _capi.lib(), _capi.ctypes
  S = len(snaps)
  nb = C.c_int64(0)
  _capi.check(lib.cnf_fp_particles_workspace(n, D, S, C.byref(nb)), "workspace")
  f64 = dict(dtype=torch.float64, device=dev)
  pos, sums = torch.full((S, n, D), 7.25, **f64), torch.full((S, 2 + D + D * D), 7.25, **f64)
  ws = torch.empty(nb.value // 8, **f64)
  g = _c_grid(grid) if (grid is not None and D >= 2) else None
  hist = None if g is None else torch.full((S, grid["n"][1], grid["n"][0]), 77, dtype=torch.int32, device=dev)
  x0d = None if x0 is None else torch.as_tensor(x0, **f64).contiguous()
  snap = (C.c_int64 * S)(*snaps)
  rc = lib.cnf_fp_particles(fp.DRIFTS[subtype], D, A, sigma, H, steps, VAR0, seed, first, n,
                            None if x0d is None else x0d.data_ptr(), snap, S, None if g is None else C.byref(g),
                            pos.data_ptr(), sums.data_ptr(), None if hist is None else hist.data_ptr(), ws.data_ptr(),
                            nb.value, None)
  assert rc == _capi.CNF_OK, rc
  torch.cuda.synchronize()
  return pos.cpu().numpy(), sums.cpu().numpy(), None if hist is None else hist.cpu().numpy().astype(np.int64)


def device_normals(dev, D, n=N, first=0, steps=STEPS, seed=SEED):
  """The particles' own normals from cnf_fill_normal, widened: z [n, steps + 1, D]"""
  from cnf_ot_amd import _capi
  R = fp.stream_stride(steps, D)
  out = torch.empty(n * R, dtype=torch.float32, device=dev)
  _capi.check(_capi.lib().cnf_fill_normal(seed, first * R, n * R, out.data_ptr(), None), "cnf_fill_normal")
  torch.cuda.synchronize()
  return fp.particle_normals(out.cpu().numpy().astype(np.float64), n, steps, D)


@pytest.fixture(scope="module")
def runs(dev):
  """Per case, computed once and left unchanged: the kernel's outputs, the restatement's positions and the tolerance"""
  out = {}
  for subtype, D in CASES:
    z = device_normals(dev, D)
    want = fp.integrate(z, subtype, A, SIGMA, H, VAR0, SNAPS)
    moved = fp.integrate(z, subtype, A, SIGMA, H, VAR0, SNAPS, x0=np.nextafter(want[0], np.inf))
    div = np.abs(moved - want).reshape(len(SNAPS), -1).max(1)            # per snapshot
    out[(subtype, D)] = dict(got=run(dev, subtype, D), want=want, div=div)
  return out


@pytest.mark.parametrize("subtype,D", CASES)
def test_paths_equal_the_restatement(runs, subtype, D):
  r = runs[(subtype, D)]
  pos, want = r["got"][0], r["want"]
  assert pos.shape == want.shape == (len(SNAPS), N, D) and np.isfinite(pos).all()
  for s, k in enumerate(SNAPS):
    tol = np.maximum(64.0 * r["div"][s], 1e-13 * np.maximum(1.0, np.abs(want[s])))
    err = np.abs(pos[s] - want[s])
    print(f"[{subtype} D={D} step {k}] max |x| {np.abs(want[s]).max():.3g}  one-ulp divergence {r['div'][s]:.3e}  "
          f"kernel error {err.max():.3e}  (bound {tol.max():.3e})")
    assert (err <= tol).all(), (subtype, D, k, float(err.max()))
  assert np.array_equal(pos[0], want[0])                                  # the start is one exact product


@pytest.mark.parametrize("subtype,D", CASES)
def test_sums_and_histogram_of_the_kernels_own_positions(dev, runs, subtype, D):
  from cnf_ot_amd import _capi
  pos, sums, hist = runs[(subtype, D)]["got"]
  grid = GRID if D >= 2 else None
  want_sums, want_hist = fp.stats(pos, grid)
  scale = np.maximum(fp.abs_sums(pos), 1e-300)
  assert np.array_equal(sums[:, :2], want_sums[:, :2]) and (sums[:, 0] == N).all()
  rel = float((np.abs(sums - want_sums) / scale).max())
  print(f"[{subtype} D={D}] sums: {rel:.2e} of sum |term|")
  assert rel <= 1e-12
  if grid is not None:
    assert np.array_equal(hist, want_hist)
    inside = want_hist.sum((1, 2))
    assert (inside > 0).all() and (inside < N).all()                      # some particles lie outside the grid
  # cnf_point_stats on the same points as float32
  lib, C = _capi.lib(), _capi.ctypes
  S = len(SNAPS)
  pts = torch.as_tensor(pos, device=dev).to(torch.float32).contiguous()
  nb = C.c_int64(0)
  _capi.check(lib.cnf_fp_particles_workspace(N, D, S, C.byref(nb)), "workspace")
  ws = torch.empty(nb.value // 8, dtype=torch.float64, device=dev)
  s2 = torch.full((S, 2 + D + D * D), 7.25, dtype=torch.float64, device=dev)
  h2 = None if grid is None else torch.full((S, 5, 7), 77, dtype=torch.int32, device=dev)
  g = None if grid is None else _c_grid(grid)
  rc = lib.cnf_point_stats(pts.data_ptr(), N, D, S, None if g is None else C.byref(g), s2.data_ptr(),
                           None if h2 is None else h2.data_ptr(), ws.data_ptr(), nb.value, None)
  assert rc == _capi.CNF_OK
  torch.cuda.synchronize()
  p32 = pts.cpu().numpy().astype(np.float64)
  want_sums, want_hist = fp.stats(p32, grid)
  s2 = s2.cpu().numpy()
  assert np.array_equal(s2[:, :2], want_sums[:, :2])
  assert float((np.abs(s2 - want_sums) / np.maximum(fp.abs_sums(p32), 1e-300)).max()) <= 1e-12
  if grid is not None:
    assert np.array_equal(h2.cpu().numpy().astype(np.int64), want_hist)


@pytest.mark.parametrize("subtype,D", [("lorenz", 3), ("ou", 5)])
def test_split_ensemble(dev, runs, subtype, D):
  pos, sums, hist = runs[(subtype, D)]["got"]
  a = run(dev, subtype, D, n=437, first=0)
  b = run(dev, subtype, D, n=563, first=437)
  assert np.array_equal(np.concatenate([a[0], b[0]], 1), pos)
  assert np.array_equal(a[2] + b[2], hist)
  assert np.array_equal((a[1] + b[1])[:, :2], sums[:, :2])
  rel = float((np.abs(a[1] + b[1] - sums) / np.maximum(fp.abs_sums(pos), 1e-300)).max())
  assert rel <= 1e-12, rel


@pytest.mark.parametrize("subtype,D", [("lorenz", 3), ("gradient", 2)])
def test_two_calls_are_bit_identical(dev, runs, subtype, D):
  again = run(dev, subtype, D)
  for x, y in zip(again, runs[(subtype, D)]["got"]):
    assert np.array_equal(x, y)


@pytest.mark.parametrize("subtype,D", [("ou", 2), ("lorenz", 3)])
def test_non_finite_start(dev, runs, subtype, D):
  x0 = runs[(subtype, D)]["want"][0].copy()
  base = run(dev, subtype, D, x0=x0)
  assert np.array_equal(base[0], runs[(subtype, D)]["got"][0])            # the drawn start given back: the same paths
  x0[300], x0[901] = np.nan, np.inf
  pos, sums, hist = run(dev, subtype, D, x0=x0)
  keep = np.ones(N, dtype=bool)
  keep[[300, 901]] = False
  assert (sums[:, 0] == N - 2).all() and (sums[:, 1] == 2).all()
  assert np.array_equal(pos[:, keep], base[0][:, keep])
  assert not np.isfinite(pos[:, ~keep]).all(2).any()
  want_sums, want_hist = fp.stats(pos, GRID)                              # (stats leaves the non-finite rows out)
  assert np.array_equal(hist, want_hist) and np.array_equal(hist, fp.stats(base[0][:, keep], GRID)[1])
  assert float((np.abs(sums - want_sums) / np.maximum(fp.abs_sums(pos), 1e-300)).max()) <= 1e-12
  assert np.isfinite(sums).all()


def test_ou_statistics_on_the_device(dev):
  from cnf_ot_amd import applications as app
  T = OU["n_steps"] * OU["h"]
  times = [k * OU["h"] for k in OU["snaps"]]
  res = app.fp_reference_particles(OU["D"], T, OU["a"], OU["sigma"], "ou", times, n_particles=OU["N"], h=OU["h"],
                                   seed=OU_SEED, var0=OU["var0"])
  assert res["hist"] is None and res["density"] is None and not bool(res["bad"].any())
  ou_check(res["count"].cpu().numpy(), res["mean"].cpu().numpy(), res["cov"].cpu().numpy(), "kernel")
  assert app.fp_reference_particles(OU["D"], T, OU["a"], OU["sigma"], "ou", times[:2], n_particles=OU["N"], h=OU["h"],
                                    seed=OU_SEED, var0=OU["var0"])["sums"].equal(res["sums"][:2])    # same paths


def _rel(a, b):
  return abs(a - b) / max(abs(b), 1e-300)


@pytest.mark.parametrize("sub,dim", [("gradient", 2), ("lorenz", 3)])
def test_evaluate_fp_path_equals_its_composition(dev, sub, dim):
  from cnf_ot_amd import FlowConfig, Params, applications as app, solvers, utils
  from cnf_ot_amd.distributed import Shard
  config = solvers.load_config(overrides={"general": {"type": "fp", "dim": dim}, "fp": {"velocity_field_type": sub}})
  f = config["fp"]
  model = solvers.build_model(config)
  params = Params.random(FlowConfig(dim=dim), 0.2, seed=4, device=dev)
  n, h, seed = 8192, 0.01, 5
  res = solvers.evaluate_fp_path(config, model, params, n_particles=n, h=h, seed=seed)
  assert set(res) == {"times", "mean_err", "cov_rel_err", "tv", "tv_floor", "density_sq_err", "bad"}
  st = solvers.figure_settings(config)
  ts = np.rint(st["t_array"] / h) * h
  S = len(ts)
  assert res["times"] == [float(t) for t in ts] and all(v is None or len(v) == S for v in res.values())
  grid = utils.field_grid(st["domain_range"], 100)
  flow = utils.point_stats(torch.stack([model.apply.sample(params, cond=float(t), seed=seed, sample_shape=(n,))
                                        for t in ts]), grid)
  whole = app.fp_reference_particles(dim, f["T"], f["a"], f["sigma"], sub, ts, n, h, seed, grid=grid)
  halves = [app.fp_reference_particles(dim, f["T"], f["a"], f["sigma"], sub, ts, n, h, seed, grid=grid,
                                       shard=Shard(r, 2), all_reduce=False) for r in (0, 1)]
  assert (halves[0]["hist"] + halves[1]["hist"]).equal(whole["hist"])
  rho = utils.eulerian_fields(model, params, grid, ts, rho=True)["rho"].double() if dim == 2 else None
  assert (res["density_sq_err"] is None) == (dim != 2)
  for s in range(S):
    want = {"mean_err": float(torch.linalg.norm(flow["mean"][s] - whole["mean"][s])),
            "cov_rel_err": float(torch.linalg.norm(flow["cov"][s] - whole["cov"][s]) / torch.linalg.norm(whole["cov"][s])),
            "tv": float(0.5 * (flow["hist"][s] - whole["hist"][s]).abs().sum()) / n,
            "tv_floor": float(0.5 * (halves[0]["hist"][s] - halves[1]["hist"][s]).abs().sum()) / (n // 2),
            "bad": float(whole["bad"][s])}
    if dim == 2:
      want["density_sq_err"] = float(((rho[s] - whole["density"][s].reshape(-1)) ** 2).sum())
    print(f"[evaluate_fp_path {sub} t={ts[s]:.2f}] " + " ".join(f"{k} {res[k][s]:.4e}" for k in want))
    for k, v in want.items():
      # the moments of the whole ensemble and of its two halves differ in the last additions of their sums
      # (explicit Euler at h = 0.01 lets an outlier of the Lorenz ensemble overflow near t = 1: the moments there are
      # astronomically large, then NaN, on both sides alike; the outlier is counted in `bad` once it is not finite)
      same = (math.isnan(res[k][s]) and math.isnan(v)) or \
        abs(res[k][s] - v) <= 1e-9 * max(abs(v), 1.0 if k in ("mean_err", "cov_rel_err") else 0.0)
      assert same, (k, s, res[k][s], v)
    assert res["tv_floor"][s] > 0.0
  # from the flow's own start the two ensembles coincide at t = 0, up to the noise floor's scale
  fl = solvers.evaluate_fp_path(config, model, params, n_particles=n, h=h, seed=seed, start="flow")
  assert fl["times"][0] == 0.0
  assert fl["tv"][0] <= fl["tv_floor"][0] and fl["mean_err"][0] <= math.sqrt(float(flow["cov"][0].trace()) / n)
  assert fl["tv_floor"][0] > 0.0
  print(f"[evaluate_fp_path {sub} start=flow] t=0: mean_err {fl['mean_err'][0]:.3e} tv {fl['tv'][0]:.3e} "
        f"floor {fl['tv_floor'][0]:.3e}")


def test_evaluate_fp_path_is_for_fp_only(dev):
  from cnf_ot_amd import FlowConfig, Params, solvers
  config = solvers.load_config()
  assert config["general"]["type"] == "rwpo"
  with pytest.raises(ValueError):
    solvers.evaluate_fp_path(config, solvers.build_model(config), Params.random(FlowConfig(dim=2), 0.2, seed=4, device=dev))
