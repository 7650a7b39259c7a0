"""The five quantities under the reference's figures -- density on a grid, its section mean, characteristics, velocity
and score -- restated from the oracle's forward / inverse / log_prob in the reference's own order of operations
(cnf_ot/utils.py:598-798; the central differences of utils.py:324-336 and :366-381).  Test helper: no tests here.

A flow is anything with `forward(x, c)`, `inverse(y, c)`, `log_prob(y, c)` on numpy arrays and a `dtype`:
`OracleFlow` wraps the C oracle (float64, or its float32 instantiation -- "the port" -- with every step of the
restatement below in float32 too), `NumpyOracleFlow` the numpy oracle.
"""
import numpy as np

import oracle
from oracle.numpy_flow import NumpyFlow


class OracleFlow:
  def __init__(self, ocfg, params, dtype=np.float64):
    self.cfg, self.dtype = ocfg, np.dtype(dtype).type
    self.params = np.asarray(params, dtype=np.float32).astype(self.dtype)
    self.D = ocfg.D

  def forward(self, x, c):
    return oracle.forward_logdet(self.cfg, self.params, x, np.asarray([c]), dtype=self.dtype)[0]

  def inverse(self, y, c):
    return oracle.inverse_logdet(self.cfg, self.params, y, np.asarray([c]), dtype=self.dtype)[0]

  def log_prob(self, y, c):
    return oracle.log_prob(self.cfg, self.params, y, np.asarray([c]), dtype=self.dtype)


class NumpyOracleFlow:
  dtype = np.float64

  def __init__(self, params, **kw):
    self.f = NumpyFlow(np.asarray(params, dtype=np.float64), **kw)
    self.D = self.f.D

  def forward(self, x, c):
    return self.f.forward_logdet(x, np.asarray([c]))[0]

  def inverse(self, y, c):
    return self.f.inverse_logdet(y, np.asarray([c]))[0]

  def log_prob(self, y, c):
    return self.f.log_prob(y, np.asarray([c]))


def grid_points(domain_range, n, dim, axes=(0, 1), fixed=None, section_value=None, section_axis=None):
  """XY of utils.py:615-618 (XYZ of :665-669, :719-742): [ny * nx, dim] float64, point i * nx + j = (x_j, y_i)."""
  x_min, x_max, y_min, y_max = domain_range
  nx, ny = (n, n) if np.ndim(n) == 0 else n
  x = np.linspace(x_min, x_max, nx)
  y = np.linspace(y_min, y_max, ny)
  X, Y = np.meshgrid(x, y)
  cols = [np.ones((nx * ny, 1)) * (0.0 if fixed is None else np.broadcast_to(np.asarray(fixed, dtype=np.float64), (dim,))[d])
          for d in range(dim)]
  cols[axes[0]] = X.reshape(nx * ny, 1)
  cols[axes[1]] = Y.reshape(nx * ny, 1)
  if section_value is not None:
    cols[section_axis] = np.ones((nx * ny, 1)) * section_value
  return np.hstack(cols)


def log_density_on_grid(flow, t_array, domain_range, n=100, axes=(0, 1), fixed=None):
  """log_prob_fn(params, XY, cond=t_i) of utils.py:621-625, [S, ny, nx]."""
  nx, ny = (n, n) if np.ndim(n) == 0 else n
  XY = grid_points(domain_range, n, flow.D, axes, fixed).astype(flow.dtype)
  return np.stack([flow.log_prob(XY, flow.dtype(t)).reshape(ny, nx) for t in t_array])


def density_on_grid(flow, t_array, domain_range, n=100, axes=(0, 1), fixed=None, section=None, section_axis=None):
  """exp(log_prob) on the grid; with sections plot_proj_density's loop (utils.py:716-745): prob += exp(...) per
  section, then prob /= len(section).  [S, ny, nx]."""
  nx, ny = (n, n) if np.ndim(n) == 0 else n
  if section is None:
    return np.exp(log_density_on_grid(flow, t_array, domain_range, n, axes, fixed))
  out = []
  for t in t_array:
    prob = np.zeros((ny, nx))
    for v in section:
      XYZ = grid_points(domain_range, n, flow.D, axes, fixed, v, section_axis).astype(flow.dtype)
      prob += np.exp(flow.log_prob(XYZ, flow.dtype(t))).reshape(ny, nx)
    prob /= len(section)
    out.append(prob)
  return np.stack(out)


def trajectories(flow, r0, t_array, t0=0.0):
  """xi = inverse_fn(params, r_, t0); r_ = forward_fn(params, xi, t) per t (utils.py:619, 626-627).  [S, N, D]."""
  xi = flow.inverse(np.asarray(r0, dtype=flow.dtype), flow.dtype(t0))
  return np.stack([flow.forward(xi, flow.dtype(t)) for t in t_array])


def _velocity_from(flow, xi, t, dt):
  t, dt = flow.dtype(t), flow.dtype(dt)
  half = flow.dtype(0.5) * dt
  r1 = flow.forward(xi, t - half)
  r2 = flow.forward(xi, t + half)
  return (r2 - r1) / dt                     # utils.py:330-337


def trajectory_velocity(flow, r0, t_array, t0=0.0, dt=0.01):
  xi = flow.inverse(np.asarray(r0, dtype=flow.dtype), flow.dtype(t0))
  return np.stack([_velocity_from(flow, xi, t, dt) for t in t_array])


def velocity_field(flow, pts, t_array, dt=0.01):
  """v(r, t) = (F(xi, t + dt/2) - F(xi, t - dt/2)) / dt, xi = F^-1(r, t).  [S, N, D]."""
  pts = np.asarray(pts, dtype=flow.dtype)
  return np.stack([_velocity_from(flow, flow.inverse(pts, flow.dtype(t)), t, dt) for t in t_array])


def score_field(flow, pts, t_array, dx=0.01):
  """(log_prob(r + dx/2 e_d) - log_prob(r - dx/2 e_d)) / dx (utils.py:366-381).  [S, N, D]."""
  pts = np.asarray(pts, dtype=flow.dtype)
  dx = flow.dtype(dx)
  half = flow.dtype(0.5) * dx
  out = np.empty((len(t_array),) + pts.shape, dtype=flow.dtype)
  for j, t in enumerate(t_array):
    for d in range(pts.shape[1]):
      e = np.zeros(pts.shape[1], dtype=flow.dtype)
      e[d] = half
      out[j, :, d] = (flow.log_prob(pts + e, flow.dtype(t)) - flow.log_prob(pts - e, flow.dtype(t))) / dx
  return out
