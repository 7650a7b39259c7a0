"""Mirror of cnf_ot/utils.py, in three parts:
  - its two Monte-Carlo evaluators (:311-389), the callers that define BASELINE's benchmark shape: 10 000 time-slices x
    65 536 samples.  The reference issues 2-3 jitted sample calls (+ 2*dim log_prob calls) per slice from a Python
    loop; here a chunk of slices is ONE fused launch (grid over (slice, sample tile)) that returns one sum per slice;
  - the arrays under its figures (:598-798): density, velocity and score fields, trajectories, and `point_stats`;
  - the distances between two point clouds (mmd2, mmd_permutation_test, sinkhorn, sliced_wasserstein and their helpers), which live in
    `two_sample` and are re-exported here, as are the interaction energy of one cloud (`interaction`) and the kernel
    Stein discrepancy of a cloud against a score and its wild-bootstrap test (`stein`) and the kernel density estimate of a cloud with its score
    (`kde`).
"""
from typing import Optional

import numpy as np
import torch

from . import _capi
from .applications import _spec, _stats_buffers, stats_from_sums, stats_grid
from .distributed import Shard, all_reduce_sums, current_shard, shard_range
from .flows import _OnDevice, _stream_ptr
from .two_sample import (  # noqa: F401
    MEDIAN_BANDWIDTH_FACTORS, median_bandwidths, mmd_spec, mmd_check_shapes, mmd2_from_sums, mmd2,
    PERM_MIN_VECTORS, PERM_MAX_VECTORS, PERM_MAX_POINTS, permutation_labels, pack_labels, mmd_perm_check_shapes,
    permutation_p_value, mmd_permutation_test,
    SINKHORN_MAX_ITERS, SINKHORN_MAX_POINTS, sinkhorn_check_shapes, sinkhorn_check_schedule, sinkhorn_schedule, sinkhorn,
    SLICED_MAX_PROJ, SLICED_MAX_POINTS, SLICED_WORKSPACE_BYTES, sliced_directions, sliced_check_shapes, sliced_group,
    sliced_wasserstein,
    KNN_MAX_K, KNN_MAX_POINTS, knn_check_shapes, knn, knn_estimates, knn_divergence, knn_entropy)
from .interaction import (  # noqa: F401
    INTERACTION_KINDS, INTERACTION_MAX_TERMS, INTERACTION_MAX_POINTS, interaction_spec, interaction_check_shapes,
    interaction_energy, interaction_field, interaction_force_vjp)
from .stein import (  # noqa: F401
    STEIN_KINDS, STEIN_MAX_TERMS, STEIN_MAX_POINTS, stein_spec, stein_check_shapes, ksd,
    STEIN_BOOT_MIN_VECTORS, STEIN_BOOT_MAX_VECTORS, rademacher_signs, stein_boot_check_shapes, ksd_bootstrap_test)
from .kde import (  # noqa: F401
    KDE_MAX_BW, KDE_MAX_POINTS, kde_spec, kde_check_shapes, kde_bandwidths, kde)


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
