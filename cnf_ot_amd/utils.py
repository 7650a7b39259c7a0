"""Mirror of the two Monte-Carlo evaluators of cnf_ot/utils.py (:311-389), the
callers that define BASELINE's benchmark shape: 10 000 time-slices x 65 536
samples.  The reference issues 2-3 jitted sample calls (+ 2*dim log_prob calls)
per slice from a Python loop; here a chunk of slices is ONE fused launch
(grid over (slice, sample tile)) that returns one sum per slice.
"""
from typing import Optional

import numpy as np
import torch

from . import _capi
from .applications import _spec
from .distributed import Shard, all_reduce_sums, current_shard, shard_range


def _model_of(fn_or_model):
  if hasattr(fn_or_model, "terms_backend"):
    return fn_or_model
  owner = getattr(fn_or_model, "__self__", None)      # model.apply.sample is a bound method
  if owner is not None and hasattr(owner, "_m"):
    return owner._m
  raise TypeError("expected a cnf_ot_amd FlowModel or one of its model.apply functions")


def _mc_energy(model, params, rng, spec, batch_size, t_array, dim, slices_per_launch, shard):
  shard = shard if shard is not None else current_shard()
  be = model.terms_backend(params)
  start, count = shard_range(batch_size, shard)
  total = torch.zeros(1, dtype=torch.float64, device=be.device)
  t_array = np.asarray(t_array, dtype=np.float32)
  for k0 in range(0, len(t_array), slices_per_launch):
    ts = t_array[k0:k0 + slices_per_launch]
    # slice k draws its own noise (the key split of utils.py:328): samples
    # [k*batch_size, (k+1)*batch_size) of the seed's stream; this rank's block of each
    if hasattr(be, "loss_terms_seeded"):      # HIP engine: noise is drawn inside the kernel, never in HBM
      total += be.loss_terms_seeded(spec, rng, ts, count, first_sample=k0 * batch_size + start,
                                    slice_stride=batch_size).sum()
      continue
    noise = torch.empty(len(ts) * count, dim, dtype=torch.float32, device=be.device)
    for j in range(len(ts)):
      noise[j * count:(j + 1) * count] = be.normal(rng, count, first_sample=(k0 + j) * batch_size + start)
    total += be.loss_terms(spec, noise, ts, count, False).sum()
  total = all_reduce_sums(total, shard)
  # e_kin += mean(velocity**2) / 2 per slice; return e_kin / t_size * dim   (utils.py:338-340)
  return total[0] / (batch_size * dim) / 2 / len(t_array) * dim


def calc_kinetic_energy(sample_fn, params, rng, batch_size: int = 65536, t_size: int = 10000, dim: int = 1,
                        slices_per_launch: int = 1024, shard: Optional[Shard] = None):
  """cnf_ot/utils.py:311-340 (dt = 0.01 hard-coded there, :324)."""
  model = _model_of(sample_fn)
  t_array = np.linspace(0.0, 1.0, t_size)
  return _mc_energy(model, params, rng, _spec(_capi.TERM_KINETIC, dt=0.01), batch_size, t_array, dim,
                    slices_per_launch, shard)


def calc_score_kinetic_energy(sample_fn, log_prob_fn, params, T: float = 1, beta: float = 1, dim: int = 1,
                              rng=0, batch_size: int = 65536, t_size: int = 10000,
                              slices_per_launch: int = 1024, shard: Optional[Shard] = None):
  """cnf_ot/utils.py:343-389 (dt = dx = 0.01 hard-coded, :360,378)."""
  model = _model_of(sample_fn)
  t_array = np.linspace(0.0, T, t_size)
  spec = _spec(_capi.TERM_KINETIC_SCORE, dt=0.01, dx=0.01, coef=1.0 / beta)
  return _mc_energy(model, params, rng, spec, batch_size, t_array, dim, slices_per_launch, shard)


# ---- the arrays under the reference's figures (cnf_ot/utils.py:598-798, called from solvers.py:309-493) -------------
# plot_density_and_trajectory, plot_high_dim_density_and_trajectory, plot_proj_density, plot_velocity_field and
# plot_traj_and_velocity evaluate the flow one time (and one section) per call and draw the result; the functions below
# return the tensors and draw nothing.  Each is ONE fused launch over all times (cnf_eulerian_fields /
# cnf_trajectories); where the fused kernel does not apply (dim > 14, periodized) -- or with fused=False -- the same
# result is composed from model.apply.log_prob / inverse / forward call by call.  A grid has no input tensor whose
# dtype could select the float64 kernels the way model.apply does: these functions take dtype= instead.

def field_grid(domain_range, n=100, axes=(0, 1), fixed=None, section=None, section_axis=None):
  """A regular grid of data space, as the reference's figures lay it out: meshgrid(linspace(x_min, x_max, nx),
  linspace(y_min, y_max, ny)) over the event axes `axes`, point i * nx + j = (x_j, y_i) (utils.py:615-618); the other
  coordinates `fixed` (a number or [D] values, default 0: the z = 3 of utils.py:665-669), and optionally `section`
  values of `section_axis` (plot_proj_density's linspace(-5, 5, 11), utils.py:714).  n: an int or (nx, ny)."""
  x_min, x_max, y_min, y_max = (float(v) for v in domain_range)
  nx, ny = (int(n), int(n)) if np.ndim(n) == 0 else (int(n[0]), int(n[1]))
  if section is not None and section_axis is None:
    raise ValueError("section needs section_axis")
  return {"domain_range": (x_min, x_max, y_min, y_max), "n": (nx, ny), "axes": (int(axes[0]), int(axes[1])),
          "fixed": fixed, "section": None if section is None else np.asarray(section, dtype=np.float64).reshape(-1),
          "section_axis": None if section_axis is None else int(section_axis), "_tensors": {}}


def _fixed_vector(g, dim):
  f = g["fixed"]
  f = np.zeros(dim) if f is None else np.asarray(f.cpu() if torch.is_tensor(f) else f, dtype=np.float64)
  return np.full(dim, float(f)) if f.ndim == 0 else f.reshape(-1)


def field_grid_points(g, dim, k=None) -> np.ndarray:
  """The [ny * nx, dim] float64 points of a `field_grid` (section value k, if it has sections), in the reference's
  meshgrid + hstack order."""
  x_min, x_max, y_min, y_max = g["domain_range"]
  nx, ny = g["n"]
  X, Y = np.meshgrid(np.linspace(x_min, x_max, nx), np.linspace(y_min, y_max, ny))
  pts = np.tile(_fixed_vector(g, dim), (nx * ny, 1))
  pts[:, g["axes"][0]] = X.reshape(-1)
  pts[:, g["axes"][1]] = Y.reshape(-1)
  if g["section"] is not None:
    pts[:, g["section_axis"]] = g["section"][0 if k is None else k]
  return pts


def _engine_grid(g, dim):
  """`field_grid` -> the grid argument of FlowEngine.eulerian_fields (lo + index * step: numpy.linspace's arithmetic)."""
  x_min, x_max, y_min, y_max = g["domain_range"]
  nx, ny = g["n"]
  step = lambda lo, hi, n: (hi - lo) / (n - 1) if n > 1 else 0.0
  return {"lo": (x_min, y_min), "step": (step(x_min, x_max, nx), step(y_min, y_max, ny)), "n": (nx, ny),
          "axes": g["axes"], "fixed": _fixed_vector(g, dim), "section": g["section"], "section_axis": g["section_axis"]}


def _grid_tensors(g, dim, dev, dtype):
  """The point tensors of a `field_grid`, one per section, for the composition: built and uploaded on first use and
  kept with the grid, so that a grid made once and passed to many calls costs its upload once."""
  key = (dim, str(dev), dtype)
  cache = g.setdefault("_tensors", {})
  if key not in cache:
    n_sec = 1 if g["section"] is None else len(g["section"])
    cache[key] = [torch.as_tensor(field_grid_points(g, dim, k)).to(device=dev, dtype=dtype)
                          for k in range(n_sec)]
  return cache[key]


def _is_grid(p):
  return isinstance(p, dict) and "domain_range" in p


def _times_of(t_array):
  return np.asarray(t_array.cpu() if torch.is_tensor(t_array) else t_array, dtype=np.float64).reshape(-1)


def _cond_of(t, dtype):
  """A time as model.apply takes it for `dtype` points: the float32 kernels see float32(t)."""
  return float(np.float32(t)) if dtype == torch.float32 else float(t)


def _eulerian(model, params, pts_or_grid, t_array, dtype, fused, exact_score=False, **want):
  if exact_score and want.get("score"):
    return _eulerian_exact_score(model, params, pts_or_grid, t_array, dtype, fused, **want)
  be = model.terms_backend(params)
  dim = model.cfg.dim
  ts = _times_of(t_array)
  if _is_grid(pts_or_grid):
    g, pts = pts_or_grid, None
    dtype = torch.float32 if dtype is None else dtype
  else:
    p = pts_or_grid if torch.is_tensor(pts_or_grid) else torch.as_tensor(np.asarray(pts_or_grid))
    g, pts = None, be._points(p if dtype is None else p.to(dtype), "fields", keep_f64=True)
    dtype = pts.dtype
  if fused:
    res = be.eulerian_fields(ts, pts=pts, grid=None if g is None else _engine_grid(g, dim), dtype=dtype, **want)
    if res is not None:
      return res
  return _eulerian_composed(model, params, be, g, pts, ts, dtype, **want)


def _eulerian_exact_score(model, params, pts_or_grid, t_array, dtype, fused, score=True, dx=None, **others):
  """The score entry from cnf_score (FlowEngine.score: one launch over all times, the points shared), every other
  field as without the flag.  Refusals come first and nothing falls back to the difference quotient: it is another
  quantity."""
  be = model.terms_backend(params)
  dim = model.cfg.dim
  if _is_grid(pts_or_grid):
    if pts_or_grid["section"] is not None and len(pts_or_grid["section"]) > 1:
      raise ValueError("a mean over several sections is defined for the density alone")
    pts = None
  else:      # (as without the flag: the points' own dtype stands where dtype= is not given)
    pts = pts_or_grid if torch.is_tensor(pts_or_grid) else torch.as_tensor(np.asarray(pts_or_grid))
    dtype = pts.dtype if dtype is None else dtype
  if dtype == torch.float64:
    raise _capi.CnfError(_capi.CNF_ERR_UNSUPPORTED, "cnf_score (the backward kernels are float32)")
  pts = _grid_tensors(pts_or_grid, dim, be.device, torch.float32)[0] if pts is None else pts.to(torch.float32)
  ts = _times_of(t_array)
  res = {"score": be.score(pts, ts, shared=True).reshape(len(ts), -1, dim)} if len(ts) else \
    {"score": torch.empty(0, len(pts), dim, dtype=torch.float32, device=be.device)}
  if any(others.get(k) for k in ("rho", "logp", "vel")):
    res.update(_eulerian(model, params, pts_or_grid, t_array, dtype, fused, **others))
  return res


def _eulerian_composed(model, params, be, g, pts, ts, dtype, rho=False, logp=False, vel=False, score=False, dt=0.01,
                       dx=0.01):
  """The same fields from the public flow calls, one time (and one section) per call -- the reference's own loops."""
  dim, dev = model.cfg.dim, be.device
  n_sec = 1 if g is None or g["section"] is None else len(g["section"])
  if n_sec > 1 and (logp or vel or score):
    raise ValueError("a mean over several sections is defined for the density alone")
  secs = [pts] if g is None else _grid_tensors(g, dim, dev, dtype)
  N = secs[0].shape[0]
  S = len(ts)
  res = {}
  if rho:
    res["rho"] = torch.empty(S, N, dtype=dtype, device=dev)
  if logp:
    res["logp"] = torch.empty(S, N, dtype=dtype, device=dev)
  if vel:
    res["vel"] = torch.empty(S, N, dim, dtype=dtype, device=dev)
  if score:
    res["score"] = torch.empty(S, N, dim, dtype=dtype, device=dev)
  for j, t in enumerate(ts):
    c = _cond_of(t, dtype)
    if rho or logp:
      acc = torch.zeros(N, dtype=torch.float64, device=dev)
      for p in secs:
        lp = model.apply.log_prob(params, p, cond=c)
        acc += torch.exp(lp.double())
      if logp:
        res["logp"][j] = lp
      if rho:
        res["rho"][j] = (acc / n_sec).to(dtype)
    if vel:
      xi = model.apply.inverse(params, secs[0], c)
      h = torch.tensor(0.5 * dt, dtype=dtype)
      cm, cp = torch.tensor(c, dtype=dtype) - h, torch.tensor(c, dtype=dtype) + h
      res["vel"][j] = (model.apply.forward(params, xi, float(cp)) - model.apply.forward(params, xi, float(cm))) * \
        float(torch.tensor(1.0, dtype=dtype) / torch.tensor(dt, dtype=dtype))
    if score:
      if dtype == torch.float32:
        res["score"][j] = be.logprob_fd(secs[0], c, dx)
      else:
        for d in range(dim):
          e = torch.zeros(dim, dtype=dtype, device=dev)
          e[d] = 0.5 * dx
          res["score"][j, :, d] = (model.apply.log_prob(params, secs[0] + e, cond=c)
                                   - model.apply.log_prob(params, secs[0] - e, cond=c)) * (1.0 / dx)
  return res


def eulerian_fields(model, params, pts_or_grid, t_array, rho=False, logp=False, vel=False, score=False, dt: float = 0.01,
                    dx: float = 0.01, dtype=None, fused=True, exact_score=False) -> dict:
  """Several fields at the same points and times from ONE launch: a dict with the entries asked for -- "rho" and
  "logp" [S, N], "vel" and "score" [S, N, D] -- as `density_on_grid`, `velocity_field` and `score_field` define them
  (a monitoring pass during training: density, velocity and score on one grid).  pts_or_grid: [N, D] points or a
  `field_grid`; with several sections only rho is defined.  exact_score=True: the score entry is the derivative
  grad_x log_prob itself (`score_field(exact=True)`: a launch of its own, dx ignored), the other entries come from
  the fused launch as before."""
  model = _model_of(model)
  if not (rho or logp or vel or score):
    raise ValueError("eulerian_fields: ask for at least one field")
  return _eulerian(model, params, pts_or_grid, t_array, dtype, fused, exact_score=exact_score, rho=rho, logp=logp,
                   vel=vel, score=score, dt=dt, dx=dx)


def density_on_grid(log_prob_fn_or_model, params, t_array, domain_range, n=100, axes=(0, 1), fixed=None, section=None,
                    section_axis=None, dtype=None, fused=True) -> torch.Tensor:
  """exp(log_prob) on the reference's grid at every time of t_array, [S, ny, nx] (n = an int: [S, n, n]): the images of
  plot_density_and_trajectory (utils.py:615-625), of plot_high_dim_density_and_trajectory with fixed=3 (:662-678) and,
  with `section` values along `section_axis`, the section mean of plot_proj_density (:711-745).  The reference shows
  the dim-3 images transposed and flipped (`.T[:, ::-1]`): that is drawing, not done here."""
  model = _model_of(log_prob_fn_or_model)
  g = field_grid(domain_range, n, axes, fixed, section, section_axis)
  rho = _eulerian(model, params, g, t_array, dtype, fused, rho=True)["rho"]
  return rho.reshape(rho.shape[0], g["n"][1], g["n"][0])


def velocity_field(model, params, pts_or_grid, t_array, dt: float = 0.01, dtype=None, fused=True) -> torch.Tensor:
  """The flow's velocity at fixed points of data space, [S, N, D]: v(r, t) = (F(xi, t + dt/2) - F(xi, t - dt/2)) / dt
  with xi = F^-1(r, t) -- the reference's central difference in t (utils.py:324-336 with general.dt) at the points of
  plot_traj_and_velocity's quiver grid (:780-794).  pts_or_grid: [N, D] points or a `field_grid`."""
  model = _model_of(model)
  return _eulerian(model, params, pts_or_grid, t_array, dtype, fused, vel=True, dt=dt)["vel"]


def score_field(model, params, pts_or_grid, t_array, dx: float = 0.01, dtype=None, fused=True, exact=False) -> torch.Tensor:
  """The score of the flow's density by the reference's central differences in x, [S, N, D]:
  (log_prob(r + dx/2 e_d) - log_prob(r - dx/2 e_d)) / dx (utils.py:366-381 with general.dx; what plot_velocity_field
  / plot_score evaluate on their grids).
  exact=True: the derivative grad_x log_prob itself, not the reference's difference quotient -- one fused forward +
  reverse pass per point (cnf_score), dx ignored, float32 (a grid's points are its float64 coordinates rounded to
  float32).  On a model cnf_score does not serve (periodized, a network other than hidden 16 / 2 layers / 5 bins,
  dim > 14) and for dtype=torch.float64 it raises CnfError(CNF_ERR_UNSUPPORTED): there is no fall-back to the
  quotient, which is a different quantity."""
  model = _model_of(model)
  return _eulerian(model, params, pts_or_grid, t_array, dtype, fused, exact_score=exact, score=True, dx=dx)["score"]


def trajectories(model, params, r_, t_array, t0: float = 0.0, with_velocity: bool = False, dt: float = 0.01, dtype=None,
                 fused=True):
  """The characteristics through the points r_ [N, D]: r(t) = F(F^-1(r_, t0), t) for t in t_array, [S, N, D]
  (utils.py:619,626-627; :670,679-680) -- with_velocity: the pair (trajectories, central-difference velocity along
  them).  float64 r_ (or dtype=torch.float64) selects the float64 kernels."""
  model = _model_of(model)
  be = model.terms_backend(params)
  r0 = be._points(r_, "trajectories", keep_f64=True)
  if dtype is not None and r0.dtype != dtype:
    r0 = r0.to(dtype)
  dtype = r0.dtype
  ts = _times_of(t_array)
  if fused:
    res = be.trajectories(r0, ts, t0, traj=True, vel=with_velocity, dt=dt)
    if res is not None:
      return res if with_velocity else res[0]
  xi = model.apply.inverse(params, r0, _cond_of(t0, dtype))
  traj = torch.stack([model.apply.forward(params, xi, _cond_of(t, dtype)) for t in ts]) if len(ts) else \
    torch.empty(0, *r0.shape, dtype=dtype, device=be.device)
  if not with_velocity:
    return traj
  vel = torch.empty_like(traj)
  for j, t in enumerate(ts):
    c = torch.tensor(_cond_of(t, dtype), dtype=dtype)
    h = torch.tensor(0.5 * dt, dtype=dtype)
    vel[j] = (model.apply.forward(params, xi, float(c + h)) - model.apply.forward(params, xi, float(c - h))) * \
      float(torch.tensor(1.0, dtype=dtype) / torch.tensor(dt, dtype=dtype))
  return traj, vel


def point_stats(pts, grid=None, axes=(0, 1)) -> dict:
  """Moments and a 2-D histogram of given points -- what a flow's own samples go through to be compared with
  applications.fp_reference_particles, by the same accumulation kernel code (cnf_point_stats): pts [S, N, D] (or
  [N, D]: S = 1) float32 on the device.  The same dictionary (applications.stats_from_sums): count, bad [S], mean
  [S, D], cov [S, D, D], sums, and with `grid` (a `field_grid` or (domain_range, n), over the event axes `axes`) hist
  [S, ny, nx] and density = hist / (N cell area), cell j centred on grid point j.  Non-finite points count as bad."""
  from .applications import _OnDevice, _stats_buffers, _stream_ptr, stats_from_sums, stats_grid
  pts = torch.as_tensor(pts)
  if pts.dim() == 2:
    pts = pts[None]
  if pts.dim() != 3 or pts.shape[1] < 1 or not 1 <= pts.shape[2] <= 14 or not 1 <= pts.shape[0] <= 64:
    raise ValueError(f"point_stats: expected [S <= 64, N >= 1, D <= 14] points, got {tuple(pts.shape)}")
  S, N, D = pts.shape
  g = stats_grid(grid, axes, D)
  if not pts.is_cuda:
    pts = pts.to(torch.device("cuda", torch.cuda.current_device()))
  pts = pts.to(torch.float32).contiguous()
  dev = pts.device
  sums, hist, ws = _stats_buffers(dev, N, D, S, g)
  with _OnDevice(dev):
    _capi.check(_capi.lib().cnf_point_stats(pts.data_ptr(), N, D, S, None if g is None else _capi.ctypes.byref(g),
                                            sums.data_ptr(), None if hist is None else hist.data_ptr(), ws.data_ptr(),
                                            ws.numel() * 8, _stream_ptr(dev)), "cnf_point_stats")
  return stats_from_sums(sums, hist, N, g, D)


# ---- kernel two-sample statistics: what compares a flow with a target that exists only as samples -------------------
# The reference: with samples of the target alone KL cannot be computed and "we need to shift to other integral
# probability metric, e.g. MMD" (tests/test_wasserstein_geodesic.py:165-169).  One fused launch over all sets
# (cnf_mmd2); composed in torch the same statistic materialises three N x M matrices.

MEDIAN_BANDWIDTH_FACTORS = (0.25, 0.5, 1.0, 2.0, 4.0)


def median_bandwidths(y, max_rows: int = 1024):
  """The median heuristic: the median pair distance of the first <= 1 024 rows of y ([M, D], or the first set of
  [S, M, D]) times (1/4, 1/2, 1, 2, 4), computed in torch (float64); a list of 5 floats."""
  y = torch.as_tensor(y)
  if y.dim() == 3:
    y = y[0]
  if y.dim() != 2 or y.shape[0] < 2:
    raise ValueError(f"median_bandwidths: expected [M >= 2, D] points, got {tuple(y.shape)}")
  med = float(torch.pdist(y[:max_rows].double()).median())
  if not (med > 0.0 and np.isfinite(med)):
    raise ValueError(f"median_bandwidths: the median pair distance is {med}")
  return [f * med for f in MEDIAN_BANDWIDTH_FACTORS]


def _mmd_sets(t, name):
  t = t if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))
  if t.dim() == 2:
    t = t[None]
  if t.dim() != 3:
    raise ValueError(f"mmd2: {name} must be [N, D] or [S, N, D], not {tuple(t.shape)}")
  return t


def mmd_spec(bandwidths, kind="gaussian"):
  """(CnfMmdSpec, the bandwidths as a list) -- ValueError for what cnf_mmd2 refuses in a spec."""
  if kind not in _capi.MMD_KINDS:
    raise ValueError(f"mmd2: kind is 'gaussian' or 'energy', not {kind!r}")
  spec = _capi.CnfMmdSpec()
  spec.kind = _capi.MMD_KINDS[kind]
  if kind == "energy":
    return spec, []
  bws = [float(b) for b in np.asarray(bandwidths.cpu() if torch.is_tensor(bandwidths) else bandwidths,
                                      dtype=np.float64).reshape(-1)]
  if not 1 <= len(bws) <= _capi.MMD_MAX_BW:
    raise ValueError(f"mmd2: between 1 and {_capi.MMD_MAX_BW} bandwidths, not {len(bws)}")
  for b in bws:
    b32 = float(np.float32(b))      # (as the kernel sees it; 1 / bw^2 must stay in float32's range)
    if not (b32 > 0.0 and np.isfinite(b32) and 1.0 / (b32 * b32) <= 3.0e38):
      raise ValueError(f"mmd2: every bandwidth must be positive and finite (in float32, with 1 / bw^2): {bws}")
  spec.n_bw = len(bws)
  for i, b in enumerate(bws):
    spec.bw[i] = b
  return spec, [float(spec.bw[i]) for i in range(len(bws))]


def mmd_check_shapes(x_shape, y_shape):
  """ValueError for sets cnf_mmd2 refuses: ([S, N, D], [S, M, D]) with S in 1..64, N, M >= 2, D in 1..14."""
  (S, N, D), (Sy, M, Dy) = x_shape, y_shape
  if S != Sy or D != Dy:
    raise ValueError(f"mmd2: x {tuple(x_shape)} and y {tuple(y_shape)} differ in the number of sets or in the dimension")
  if not 1 <= S <= _capi.MMD_MAX_SETS or not 1 <= D <= _capi.MMD_MAX_DIM or N < 2 or M < 2 or max(N, M) > 1 << 24:
    raise ValueError(f"mmd2: needs 1..{_capi.MMD_MAX_SETS} sets of 2..2^24 points of dimension 1..{_capi.MMD_MAX_DIM}, "
                     f"not x {tuple(x_shape)}, y {tuple(y_shape)}")


def mmd2_from_sums(sums, N, M):
  """The unbiased MMD^2 [S] from raw sums [S, 3] = (sxx, syy, sxy)."""
  return sums[:, 0] / (N * (N - 1.0)) + sums[:, 1] / (M * (M - 1.0)) - 2.0 * sums[:, 2] / (float(N) * M)


def mmd2(x, y, bandwidths=None, kind="gaussian", want_grad=False) -> dict:
  """The unbiased kernel two-sample statistic between the point sets x [N, D] or [S, N, D] and y [M, D] or [S, M, D]
  (set s of x against set s of y), ONE fused launch over all sets and all three pair blocks (cnf_mmd2):
    kind="gaussian": k(x, y) = sum_b exp(-|x - y|^2 / (2 bw_b^2)) over up to 8 `bandwidths` (None:
                     median_bandwidths(y)) -- MMD^2
    kind="energy":   k(x, y) = -|x - y| -- the energy distance 2 E|x - y| - E|x - x'| - E|y - y'|
  float32 on the device (float64 inputs are rounded; host inputs are uploaded).  Returns a dict: mmd2 [S] (float64),
  sums [S, 3] (the raw sxx, syy, sxy: diagonal left out), bandwidths (a list; empty for energy) and, with want_grad,
  grad [S, N, D] (float32; [N, D] for 2-D x) = d mmd2 / d x.  Two calls give the same bits.  ValueError before any
  device work for what the C ABI refuses (D outside 1..14, N or M < 2, more than 64 sets or 8 bandwidths, a bandwidth
  that is not positive and finite, an unknown kind) and for x and y that differ in S or D."""
  from .applications import _OnDevice, _stream_ptr
  x3, y3 = _mmd_sets(x, "x"), _mmd_sets(y, "y")
  mmd_check_shapes(x3.shape, y3.shape)
  if kind == "gaussian" and bandwidths is None:
    bandwidths = median_bandwidths(y3)
  spec, bws = mmd_spec(bandwidths, kind)
  S, N, D = x3.shape
  M = y3.shape[1]
  dev = x3.device if x3.is_cuda else (y3.device if y3.is_cuda else torch.device("cuda", torch.cuda.current_device()))
  x3 = x3.to(device=dev, dtype=torch.float32).contiguous()
  y3 = y3.to(device=dev, dtype=torch.float32).contiguous()
  lib, C = _capi.lib(), _capi.ctypes
  nbytes = C.c_int64(0)
  _capi.check(lib.cnf_mmd_workspace(S, N, M, D, 1 if want_grad else 0, C.byref(nbytes)), "cnf_mmd_workspace")
  ws = torch.empty(-(-nbytes.value // 8), dtype=torch.float64, device=dev)
  sums = torch.empty(S, 3, dtype=torch.float64, device=dev)
  grad = torch.empty(S, N, D, dtype=torch.float32, device=dev) if want_grad else None
  with _OnDevice(dev):
    _capi.check(lib.cnf_mmd2(C.byref(spec), S, x3.data_ptr(), N, y3.data_ptr(), M, D, sums.data_ptr(),
                             None if grad is None else grad.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream_ptr(dev)),
                "cnf_mmd2")
  out = {"mmd2": mmd2_from_sums(sums, N, M), "sums": sums, "bandwidths": bws}
  if want_grad:
    out["grad"] = grad if np.ndim(x) == 3 else grad[0]
  return out


# ---- the Sinkhorn divergence: an optimal-transport estimate between point clouds, in transport units -----------------
# Log-domain Sinkhorn on C(x, y) = |x - y|^2 / 2, debiased: S_eps(x, y) = OT_eps(x, y) - OT_eps(x, x) / 2 - OT_eps(y, y) / 2,
# with the dual potentials, the barycentric map (an estimate of the Monge map) and the gradient in x.  The iteration
# count and the eps of every iteration are inputs of the kernel (cnf_sinkhorn): the schedule below is
# the usual annealing, and `change` in the result says how far from its fixed point the recursion stopped.

SINKHORN_MAX_ITERS, SINKHORN_MAX_POINTS = 512, 1 << 20


def _sinkhorn_sets(t, name):
  t = t if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))
  if t.dim() == 2:
    t = t[None]
  if t.dim() != 3:
    raise ValueError(f"sinkhorn: {name} must be [N, D] or [S, N, D], not {tuple(t.shape)}")
  return t


def sinkhorn_check_shapes(x_shape, y_shape):
  """ValueError for sets cnf_sinkhorn refuses: ([S, N, D], [S, M, D]) with S in 1..64, N, M in 2..2^20, D in 1..14."""
  (S, N, D), (Sy, M, Dy) = x_shape, y_shape
  if S != Sy or D != Dy:
    raise ValueError(f"sinkhorn: x {tuple(x_shape)} and y {tuple(y_shape)} differ in the number of sets or in the dimension")
  if (not 1 <= S <= _capi.MMD_MAX_SETS or not 1 <= D <= _capi.MMD_MAX_DIM or min(N, M) < 2
      or max(N, M) > SINKHORN_MAX_POINTS):
    raise ValueError(f"sinkhorn: needs 1..{_capi.MMD_MAX_SETS} sets of 2..2^20 points of dimension 1..{_capi.MMD_MAX_DIM}, "
                     f"not x {tuple(x_shape)}, y {tuple(y_shape)}")


def sinkhorn_check_schedule(schedule):
  """The schedule as a list of floats -- ValueError for what cnf_sinkhorn refuses in one: no entry or more than 512, an
  eps that is not positive and finite or whose inverse leaves float32's range."""
  eps = [float(e) for e in np.asarray(schedule.cpu() if torch.is_tensor(schedule) else schedule, dtype=np.float64).reshape(-1)]
  if not 1 <= len(eps) <= SINKHORN_MAX_ITERS:
    raise ValueError(f"sinkhorn: a schedule has 1..{SINKHORN_MAX_ITERS} entries, not {len(eps)}")
  for e in eps:
    if not (e > 0.0 and np.isfinite(e) and 1.2e-38 <= 1.0 / e <= 2.0e38):
      raise ValueError(f"sinkhorn: every eps must be positive and finite, with 1 / eps in float32's range: {e}")
  return eps


def sinkhorn_schedule(x, y, eps, ratio=0.8, extra=10):
  """The annealing schedule of `sinkhorn`, a list of floats: the squared diagonal of the joint bounding box of x and y
  (all sets), times ratio^k for k = 0, 1, ... while that is > eps, then `extra` entries at eps.  ValueError for an eps
  that is not positive and finite, a ratio outside (0, 1), extra < 0, an empty schedule or more than 512 entries."""
  eps, ratio, extra = float(eps), float(ratio), int(extra)
  if not (eps > 0.0 and np.isfinite(eps)) or not 0.0 < ratio < 1.0 or extra < 0:
    raise ValueError(f"sinkhorn_schedule: needs eps > 0, 0 < ratio < 1 and extra >= 0, not {eps}, {ratio}, {extra}")
  pts = [t.detach().reshape(-1, t.shape[-1]).double() for t in (_sinkhorn_sets(x, "x"), _sinkhorn_sets(y, "y"))]
  lo = torch.minimum(pts[0].min(0).values.cpu(), pts[1].min(0).values.cpu())
  hi = torch.maximum(pts[0].max(0).values.cpu(), pts[1].max(0).values.cpu())
  v = float(((hi - lo) ** 2).sum())
  if not np.isfinite(v):
    raise ValueError("sinkhorn_schedule: the points are not finite")
  out = []
  while v > eps and len(out) + extra <= SINKHORN_MAX_ITERS:
    out.append(v)
    v *= ratio
  out += [eps] * extra
  if len(out) > SINKHORN_MAX_ITERS:
    raise ValueError(f"sinkhorn_schedule: more than {SINKHORN_MAX_ITERS} iterations (diagonal^2 {out[0]:.3g}, eps {eps}, "
                     f"ratio {ratio}, extra {extra})")
  if not out:
    raise ValueError("sinkhorn_schedule: an empty schedule (the bounding box is within eps and extra = 0)")
  return out


def sinkhorn(x, y, eps=0.05, schedule=None, want_grad=False, want_map=False, want_potentials=False) -> dict:
  """The Sinkhorn divergence S_eps between the point sets x [N, D] or [S, N, D] and y [M, D] or [S, M, D] (set s of x
  against set s of y; uniform weights, cost |x - y|^2 / 2), ONE cnf_sinkhorn call over all sets: len(schedule)
  averaged Jacobi iterations of the four potentials f, g (x against y), p (x against x), q (y against y) and a final
  pass at the last eps (the recursion: include/cnf_ot_amd.h).  schedule: the eps of every iteration (None:
  sinkhorn_schedule(x, y, eps); with a schedule `eps` is not used).  float32 on the device (float64 inputs are rounded;
  host inputs are uploaded).  Returns a dict:
    divergence [S]  (sum f* - sum p*) / N + (sum g* - sum q*) / M (float64): an estimate of W2^2 / 2
    ot_xy [S]       sum f* / N + sum g* / M, the entropic cost of x against y alone
    change [S, 2]   the largest |f* - f|, |g* - g| and |p* - p|, |q* - q| of the final pass: 0 at the fixed point
    grad            want_grad: [S, N, D] float32 ([N, D] for 2-D x), the envelope gradient of the divergence in x (the
                    potentials held fixed: exact at the fixed point); else None
    map             want_map: the barycentric map T(x_i) = sum_j pi_ij y_j / sum_j pi_ij, shaped like grad; else None
    f, g, p, q      want_potentials: [S, N], [S, M], [S, N], [S, M] float32; else None
    schedule        the list of eps used
  Two calls give the same bits, and the numbers do not depend on the want_ flags.  ValueError before any device work
  for what the C ABI refuses and for x and y that differ in S or D."""
  from .applications import _OnDevice, _stream_ptr
  x3, y3 = _sinkhorn_sets(x, "x"), _sinkhorn_sets(y, "y")
  sinkhorn_check_shapes(x3.shape, y3.shape)
  sched = sinkhorn_check_schedule(sinkhorn_schedule(x3, y3, eps) if schedule is None else schedule)
  S, N, D = x3.shape
  M = y3.shape[1]
  dev = x3.device if x3.is_cuda else (y3.device if y3.is_cuda else torch.device("cuda", torch.cuda.current_device()))
  x3 = x3.detach().to(device=dev, dtype=torch.float32).contiguous()
  y3 = y3.detach().to(device=dev, dtype=torch.float32).contiguous()
  lib, C = _capi.lib(), _capi.ctypes
  nbytes = C.c_int64(0)
  _capi.check(lib.cnf_sinkhorn_workspace(S, N, M, D, C.byref(nbytes)), "cnf_sinkhorn_workspace")
  ws = torch.empty(-(-nbytes.value // 8), dtype=torch.float64, device=dev)
  sums = torch.empty(S, 6, dtype=torch.float64, device=dev)
  grad = torch.empty(S, N, D, dtype=torch.float32, device=dev) if want_grad else None
  tmap = torch.empty(S, N, D, dtype=torch.float32, device=dev) if want_map else None
  pot = torch.empty(S, 2 * (N + M), dtype=torch.float32, device=dev) if want_potentials else None
  ptr = lambda t: None if t is None else t.data_ptr()
  with _OnDevice(dev):
    _capi.check(lib.cnf_sinkhorn(S, x3.data_ptr(), N, y3.data_ptr(), M, D, (C.c_double * len(sched))(*sched), len(sched),
                                 sums.data_ptr(), ptr(pot), ptr(grad), ptr(tmap), ws.data_ptr(), ws.numel() * 8,
                                 _stream_ptr(dev)), "cnf_sinkhorn")
  one = np.ndim(x) != 3
  f, g, p, q = (None,) * 4 if pot is None else pot.split([N, M, N, M], dim=1)
  return {"divergence": (sums[:, 0] - sums[:, 2]) / N + (sums[:, 1] - sums[:, 3]) / M,
          "ot_xy": sums[:, 0] / N + sums[:, 1] / M, "change": sums[:, 4:6],
          "grad": grad if grad is None or not one else grad[0], "map": tmap if tmap is None or not one else tmap[0],
          "f": f, "g": g, "p": p, "q": q, "schedule": sched}


# ---- the sliced Wasserstein distance: transport units between point clouds of any size, N log N per projection -------
# Both clouds are projected on P directions; along a direction optimal transport is exact and is a sort.  No eps, no
# iteration count, no debiasing; cost |.|^2 / 2 as `sinkhorn`, so for unit directions drawn uniformly SW <= W2^2 / (2 D),
# and with the coordinate axes as directions sqrt(2 w) is the exact W2 of every marginal (cnf_sliced_w2).

SLICED_MAX_PROJ, SLICED_MAX_POINTS, SLICED_WORKSPACE_BYTES = 1024, 1 << 20, 1 << 30
_SLICED_WS = {}                                  # device -> the cached workspace (grown, never shrunk)


def sliced_directions(D, P, seed=0, kind="random"):
  """Directions for `sliced_wasserstein`, [P, D] float32 on the host.  kind="random": P unit vectors, Gaussian draws of
  numpy's default_rng(seed) normalised in float64 -- a fixed function of (D, P, seed); for D = 1 the single direction
  +1 (P must be 1: the other direction, -1, gives the same value).  kind="axes": the D coordinate axes (P must be D).
  ValueError for D outside 1..14, P outside 1..1024, an unknown kind or a P the kind does not allow."""
  D, P = int(D), int(P)
  if not 1 <= D <= _capi.MMD_MAX_DIM or not 1 <= P <= SLICED_MAX_PROJ:
    raise ValueError(f"sliced_directions: needs D in 1..{_capi.MMD_MAX_DIM} and P in 1..{SLICED_MAX_PROJ}, not {D}, {P}")
  if kind == "axes":
    if P != D:
      raise ValueError(f"sliced_directions: the axes of dimension {D} are {D} directions, not {P}")
    return torch.eye(D, dtype=torch.float32)
  if kind != "random":
    raise ValueError(f"sliced_directions: kind is 'random' or 'axes', not {kind!r}")
  if D == 1:
    if P != 1:
      raise ValueError(f"sliced_directions: dimension 1 has the single direction +1, not {P}")
    return torch.ones(1, 1, dtype=torch.float32)
  g = np.random.default_rng(int(seed)).standard_normal((P, D))
  return torch.from_numpy((g / np.sqrt((g * g).sum(1, keepdims=True))).astype(np.float32))


def sliced_check_shapes(x_shape, y_shape, theta_shape=None):
  """ValueError for what cnf_sliced_w2 refuses: ([S, N, D], [S, M, D], [P, D]) with S in 1..64, N, M in 1..2^20, D in
  1..14, P in 1..1024."""
  (S, N, D), (Sy, M, Dy) = x_shape, y_shape
  if S != Sy or D != Dy:
    raise ValueError(f"sliced: x {tuple(x_shape)} and y {tuple(y_shape)} differ in the number of sets or in the dimension")
  if (not 1 <= S <= _capi.MMD_MAX_SETS or not 1 <= D <= _capi.MMD_MAX_DIM or min(N, M) < 1
      or max(N, M) > SLICED_MAX_POINTS):
    raise ValueError(f"sliced: needs 1..{_capi.MMD_MAX_SETS} sets of 1..2^20 points of dimension 1..{_capi.MMD_MAX_DIM}, "
                     f"not x {tuple(x_shape)}, y {tuple(y_shape)}")
  if theta_shape is not None and (len(theta_shape) != 2 or theta_shape[1] != D or not 1 <= theta_shape[0] <= SLICED_MAX_PROJ):
    raise ValueError(f"sliced: directions must be [P, {D}] with P in 1..{SLICED_MAX_PROJ}, not {tuple(theta_shape)}")


def _sliced_sets(t, name):
  t = t if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))
  if t.dim() == 2:
    t = t[None]
  if t.dim() != 3:
    raise ValueError(f"sliced: {name} must be [N, D] or [S, N, D], not {tuple(t.shape)}")
  return t


def sliced_group(S, N, M, D, P, want_grad, limit=SLICED_WORKSPACE_BYTES):
  """(G, bytes): the largest group of projections whose workspace (cnf_sliced_workspace) is at most `limit` bytes -- 1
  if even that is more -- and that workspace's size.  The size is linear in G, so two calls settle it."""
  lib, C = _capi.lib(), _capi.ctypes

  def size(G):
    b = C.c_int64(0)
    _capi.check(lib.cnf_sliced_workspace(S, N, M, D, G, int(want_grad), C.byref(b)), "cnf_sliced_workspace")
    return b.value
  b1 = size(1)
  G = 1 if P == 1 or b1 >= limit else max(1, min(P, 1 + (limit - b1) // (size(2) - b1)))
  return G, size(G)


def sliced_wasserstein(x, y, directions=None, n_proj=64, seed=0, want_grad=False) -> dict:
  """The sliced Wasserstein distance between the point sets x [N, D] or [S, N, D] and y [M, D] or [S, M, D] (set s of x
  against set s of y; uniform weights, cost |.|^2 / 2), ONE cnf_sliced_w2 call over all sets.  directions: [P, D]
  (None: sliced_directions(D, n_proj, seed), or the single direction of D = 1); they are used as given, not
  normalised.  float32 on the device (float64 inputs are rounded; host inputs are uploaded).  Returns a dict:
    sw [S]               the mean over the directions of the one-dimensional transport cost (float64)
    per_projection [S, P]  that cost per direction: the quantile-function integral, exact for any N and M
    max_sliced [S]       its maximum over the given directions
    directions [P, D]    the directions used, float32 on the device
    grad                 want_grad: [S, N, D] float32 ([N, D] for 2-D x), the envelope gradient of sw in x (the sorting
                         permutations held fixed: exact wherever the projected samples are distinct); else None
  The projections are processed in the largest groups whose workspace stays within 1 GiB (sliced_group); the result
  does not depend on the grouping, and two calls give the same bits.  The workspace is cached per device.  ValueError
  before any device work for what the C ABI refuses and for x, y and directions that differ in S or D."""
  from .applications import _OnDevice, _stream_ptr
  x3, y3 = _sliced_sets(x, "x"), _sliced_sets(y, "y")
  sliced_check_shapes(x3.shape, y3.shape)
  S, N, D = x3.shape
  M = y3.shape[1]
  if directions is None:
    directions = sliced_directions(D, 1 if D == 1 else n_proj, seed)
  th = directions if torch.is_tensor(directions) else torch.as_tensor(np.asarray(directions))
  sliced_check_shapes(x3.shape, y3.shape, tuple(th.shape))
  P = th.shape[0]
  dev = x3.device if x3.is_cuda else (y3.device if y3.is_cuda else torch.device("cuda", torch.cuda.current_device()))
  x3 = x3.detach().to(device=dev, dtype=torch.float32).contiguous()
  y3 = y3.detach().to(device=dev, dtype=torch.float32).contiguous()
  th = th.detach().to(device=dev, dtype=torch.float32).contiguous()
  G, nbytes = sliced_group(S, N, M, D, P, want_grad)
  ws = _SLICED_WS.get(dev)
  if ws is None or ws.numel() * 8 < nbytes:
    _SLICED_WS[dev] = None                       # (the old one is released before the new one is asked for)
    ws = _SLICED_WS[dev] = torch.empty(-(-nbytes // 8), dtype=torch.float64, device=dev)
  sums = torch.empty(S, P + 2, dtype=torch.float64, device=dev)
  grad = torch.empty(S, N, D, dtype=torch.float32, device=dev) if want_grad else None
  with _OnDevice(dev):
    _capi.check(_capi.lib().cnf_sliced_w2(S, x3.data_ptr(), N, y3.data_ptr(), M, D, th.data_ptr(), P, G, sums.data_ptr(),
                                          None if grad is None else grad.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                          _stream_ptr(dev)), "cnf_sliced_w2")
  return {"sw": sums[:, P], "per_projection": sums[:, :P], "max_sliced": sums[:, P + 1], "directions": th,
          "grad": grad if grad is None or np.ndim(x) == 3 else grad[0]}
