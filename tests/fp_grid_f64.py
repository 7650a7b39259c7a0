"""A NumPy float64 restatement of the finite-volume Fokker-Planck reference (cnf_fp_grid, applications.fp_reference_grid),
written from the scheme's statement, not from the kernel.

Grid: points x_i = x_min + i dx, y_j likewise; cell (j, i) centred on its point; arrays [ny, nx].
Flux (Scharfetter-Gummel / Chang-Cooper): B(z) = z / expm1(z) (1 - z / 2 for |z| < 1e-8), Pe = b dx / sigma with b the
normal drift at the face's midpoint (a rounded to float32 first); the east face of cell i carries
F = cL rho_i - cR rho_{i+1}, cL = sigma / dx^2 B(-Pe), cR = sigma / dx^2 B(Pe); the box's faces carry none.
Step: rho' = rho + dt ((F_w - F_e) + (G_s - G_n)).  Between output times Delta apart: n = ceil(Delta R / safety) steps
of dt = Delta / n, R the largest sum of the four coefficients that multiply a cell's own rho."""
import math

import numpy as np


def axes_of(domain, n):
  x_min, x_max, y_min, y_max = (float(v) for v in domain)
  nx, ny = (int(n), int(n)) if np.ndim(n) == 0 else (int(n[0]), int(n[1]))
  dx, dy = (x_max - x_min) / (nx - 1), (y_max - y_min) / (ny - 1)
  return x_min + np.arange(nx) * dx, y_min + np.arange(ny) * dy, dx, dy


def drift(x, y, a, subtype):
  a = float(np.float32(a))
  if subtype == "ou":
    return x * -a, y * -a
  if subtype in ("gradient", "smile"):
    q = x * x + y * y - 4.0
    return (-q * x) * a, (-q * y - (y - 1.0) * 2.0) * a
  if subtype == "nongradient":
    return x * -a - y * 0.5, y * -a + x * 0.5
  raise ValueError(subtype)


def bernoulli(z):
  z = np.asarray(z, dtype=np.float64)
  small = np.abs(z) < 1e-8
  safe = np.where(small, 1.0, z)
  with np.errstate(over="ignore"):
    return np.where(small, 1.0 - 0.5 * z, safe / np.expm1(safe))


def coefficients(domain, n, a, sigma, subtype):
  """cxL, cxR [ny, nx + 1] (face f of a row lies between cells f - 1 and f) and cyL, cyR [ny + 1, nx]; zeros on the
  box's faces."""
  x, y, dx, dy = axes_of(domain, n)
  nx, ny = x.size, y.size
  cxL, cxR = np.zeros((ny, nx + 1)), np.zeros((ny, nx + 1))
  cyL, cyR = np.zeros((ny + 1, nx)), np.zeros((ny + 1, nx))
  if nx > 1:
    xf = float(domain[0]) + (np.arange(1, nx) - 0.5) * dx
    b = drift(xf[None, :], y[:, None], a, subtype)[0] + np.zeros((ny, nx - 1))
    pe = b * dx / sigma
    cxL[:, 1:nx] = sigma / (dx * dx) * bernoulli(-pe)
    cxR[:, 1:nx] = sigma / (dx * dx) * bernoulli(pe)
  if ny > 1:
    yf = float(domain[2]) + (np.arange(1, ny) - 0.5) * dy
    b = drift(x[None, :], yf[:, None], a, subtype)[1] + np.zeros((ny - 1, nx))
    pe = b * dy / sigma
    cyL[1:ny, :] = sigma / (dy * dy) * bernoulli(-pe)
    cyR[1:ny, :] = sigma / (dy * dy) * bernoulli(pe)
  return cxL, cxR, cyL, cyR


def rate(c):
  cxL, cxR, cyL, cyR = c
  return float((((cxL[:, 1:] + cxR[:, :-1]) + cyL[1:, :]) + cyR[:-1, :]).max())


def step(rho, c, dt):
  cxL, cxR, cyL, cyR = c
  ny, nx = rho.shape
  p = np.zeros((ny + 2, nx + 2))
  p[1:-1, 1:-1] = rho
  F = cxL * p[1:-1, :-1] - cxR * p[1:-1, 1:]         # [ny, nx + 1]: face f between cells f - 1 and f
  G = cyL * p[:-1, 1:-1] - cyR * p[1:, 1:-1]         # [ny + 1, nx]
  return rho + dt * ((F[:, :-1] - F[:, 1:]) + (G[:-1, :] - G[1:, :]))


def step_count(delta, R, safety=0.9):
  return 0 if delta == 0.0 else max(1, int(math.ceil(delta * R / safety)))


def initial(domain, n, var0):
  """Exact cell averages of N(0, var0 I): a product of erf differences over the cells' edges"""
  x, y, dx, dy = axes_of(domain, n)
  s = math.sqrt(2.0 * var0)

  def avg(c, d):
    e = np.array([math.erf((v - 0.5 * d) / s) for v in c] + [math.erf((c[-1] + 0.5 * d) / s)])
    return 0.5 * (e[1:] - e[:-1]) / d

  return avg(y, dy)[:, None] * avg(x, dx)[None, :]


def statistics(rho, domain, n):
  x, y, dx, dy = axes_of(domain, n)
  X, Y = x[None, :], y[:, None]
  area = dx * dy
  return np.array([rho.sum() * area, rho.min(), (rho * X).sum() * area, (rho * Y).sum() * area,
                   (rho * X * X).sum() * area, (rho * X * Y).sum() * area, (rho * Y * Y).sum() * area])


def magnitudes(rho, domain, n):
  """The sums of the absolute terms of `statistics` (the scale a sum's rounding error is relative to); min: max rho"""
  x, y, dx, dy = axes_of(domain, n)
  X, Y = np.abs(x[None, :]), np.abs(y[:, None])
  area, r = dx * dy, np.abs(rho)
  return np.array([r.sum() * area, r.max(), (r * X).sum() * area, (r * Y).sum() * area, (r * X * X).sum() * area,
                   (r * X * Y).sum() * area, (r * Y * Y).sum() * area])


def solve(domain, n, a, sigma, subtype, times, var0=1.0, rho0=None, safety=0.9):
  """density [S, ny, nx], stats [S, 7], n_steps [S], rate"""
  c = coefficients(domain, n, a, sigma, subtype)
  R = rate(c)
  rho = initial(domain, n, var0) if rho0 is None else np.array(rho0, dtype=np.float64)
  out, counts, t_prev = [], [], 0.0
  for t in np.asarray(times, dtype=np.float64).reshape(-1):
    delta = float(t) - t_prev
    k = step_count(delta, R, safety)
    for _ in range(k):
      rho = step(rho, c, delta / k)
    out.append(rho.copy())
    counts.append(k)
    t_prev = float(t)
  dens = np.stack(out)
  return {"density": dens, "stats": np.stack([statistics(d, domain, n) for d in dens]),
          "n_steps": np.array(counts, dtype=np.int64), "rate": R, "coef": c}


def moments(stats):
  """mean [2] and cov [2, 2] of one snapshot's statistics"""
  m, _, sx, sy, sxx, sxy, syy = stats
  mean = np.array([sx / m, sy / m])
  second = np.array([[sxx, sxy], [sxy, syy]]) / m
  return mean, second - mean[:, None] * mean[None, :]


def gaussian_at_centres(domain, n, var):
  x, y, _, _ = axes_of(domain, n)
  return np.exp(-(x[None, :] ** 2 + y[:, None] ** 2) / (2.0 * var)) / (2.0 * math.pi * var)
