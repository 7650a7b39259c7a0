"""Float64 numpy restatement of the 2-D Hopf-Cole reference solution (cnf_ot/mfc/2d_WPO_ref_solution.py:60-187) that
the GPU tests compare cnf_hopf_cole_2d with, and the direct O(N^4) double sum that pins the restatement itself.

With eps = 1/beta, kappa = 1/(4 eps T), rho0 = N(0, var0 I), the y grid k dz (|k| <= n_y = round(y_range / dz)), the
z window |z_i - y_i| <= n_w dz (n_w = round(window / dz)):
  h(y)     = sum_z exp(-g(z) / (2 eps) - kappa |y - z|^2) dz^2
  rho_T(x) = exp(-g(x) / (2 eps)) sum_y exp(-kappa |x - y|^2) rho0(y) / h(y) dy^2
  score_T  = -grad g / (2 eps) - (x - m) / (2 eps T),  w0 = -(x - m0) / T + eps x,  wT = -grad g - eps score_T
  true     = -2 eps sum_y rho0(y) (log h(y) - log(4 pi eps T)) dy^2,   ic_mass = sum_y rho0(y) dy^2
`solve` sums them as two 1-D log-sum-exp passes (the kernel's order); `direct` sums each point's whole 2-D set at
once.  Both are float64 and differ only in summation order.  `a` is rounded to float32, as the C ABI carries it.
"""
import functools
import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

POTENTIALS = ("quadratic", "double_well", "obstacle")


def potential(x1, x2, subtype, a):
  """g and its gradient (potential_loss_fn, applications.py:181-191)"""
  a = float(np.float32(a))
  if subtype == "quadratic":
    return (x1 * x1 + x2 * x2) / 2, x1, x2
  if subtype == "double_well":
    sm = (x1 - a) ** 2 + (x2 - a) ** 2
    sp = (x1 + a) ** 2 + (x2 + a) ** 2
    return sm * sp / 4, ((x1 - a) * sp + (x1 + a) * sm) / 2, ((x2 - a) * sp + (x2 + a) * sm) / 2
  if subtype == "obstacle":
    v = 50 * np.exp(-(x1 * x1 + x2 * x2) / 2)
    return v, -x1 * v, -x2 * v
  raise ValueError(subtype)


def grids(dz, window, y_range):
  ny, nw = round(y_range / dz), round(window / dz)
  y = np.arange(-ny, ny + 1) * dz
  z = np.arange(-(ny + nw), ny + nw + 1) * dz
  return ny, nw, y, z


def _lse_rows(a, carry=None, src=None, chunk=32):
  """log-sum-exp over the last axis of a [R, J, K] (built by `a(rows)`), with the weighted means of src [K] and of
  carry [R, K]; rows in chunks to bound the memory"""
  L, M, C = [], [], []
  for r0 in range(0, a.rows, chunk):
    rows = slice(r0, min(a.rows, r0 + chunk))
    t = a(rows)
    m = t.max(axis=2, keepdims=True)
    e = np.exp(t - m)
    s = e.sum(axis=2)
    L.append(m[..., 0] + np.log(s))
    if src is not None:
      M.append((e * src).sum(axis=2) / s)
    if carry is not None:
      C.append((e * carry[rows, None, :]).sum(axis=2) / s)
  cat = lambda v: np.concatenate(v) if v else None
  return cat(L), cat(M), cat(C)


class _Terms:
  def __init__(self, rows, fn):
    self.rows, self.fn = rows, fn

  def __call__(self, rows):
    return self.fn(rows)


def _window_pass(lw, nw, kappa, dz):
  """sum over the window: lw [R, Nz] -> [R, Ny], destination j reading sources j .. j + 2 nw"""
  lk = -kappa * ((np.arange(2 * nw + 1) - nw) * dz) ** 2
  sw = sliding_window_view(lw, 2 * nw + 1, axis=1)
  return _lse_rows(_Terms(lw.shape[0], lambda rows: sw[rows] + lk))[0]


def _free_pass(lw, src, dst, kappa, carry=None, means=False):
  """sum over every source: lw [R, S] at coordinates src -> [R, len(dst)], with the means"""
  lk = -kappa * (dst[:, None] - src[None, :]) ** 2
  return _lse_rows(_Terms(lw.shape[0], lambda rows: lw[rows, None, :] + lk), carry, src if means else None)


def _to_outputs(lw, y, x1, x2, kappa, means):
  LC, MC, _ = _free_pass(lw, y, x1, kappa, means=means)            # [y2, x1]
  L, M2, M1 = _free_pass(LC.T, y, x2, kappa, carry=MC.T if means else None, means=means)   # [x1, x2]
  return L.T, None if M1 is None else M1.T, None if M2 is None else M2.T


def _log_rho0(y1, y2, var0):
  return -(y1 ** 2 + y2 ** 2) / (2 * var0) - math.log(2 * math.pi * var0)


def _finish(out, X1, X2, L, m, m0, subtype, a, eps, T, dz):
  g, g1, g2 = potential(X1, X2, subtype, a)
  out["log_rho_T"] = L + 2 * math.log(dz) - g / (2 * eps)
  x, gr = np.stack([X1, X2], -1), np.stack([g1, g2], -1)
  score = -gr / (2 * eps) - (x - m) / (2 * eps * T)
  out["score_T"], out["wT"] = score, -gr - eps * score
  out["w0"] = -(x - m0) / T + eps * x
  return out


@functools.lru_cache(maxsize=4)
def _log_h(beta, T, a, subtype, dz, window, y_range):
  """-g / (2 eps) on the z grid [z2, z1] and log h on the y grid [y2, y1] (cached: the tests ask for several output
  grids of one problem)"""
  eps, kappa = 1.0 / beta, beta / (4.0 * T)
  _, nw, _, z = grids(dz, window, y_range)
  Z1, Z2 = np.meshgrid(z, z)
  lg = -potential(Z1, Z2, subtype, a)[0] / (2 * eps)               # [z2, z1]
  LA = _window_pass(lg, nw, kappa, dz)                             # [z2, y1]
  return lg, _window_pass(LA.T, nw, kappa, dz).T + 2 * math.log(dz)   # [y2, y1]


def solve(T, beta, a, subtype, x1, x2=None, var0=None, dz=0.01, window=6.0, y_range=4.0):
  """The separable restatement: dict of log_rho_T [n2, n1], score_T / w0 / wT [n2, n1, 2], true_val, ic_mass."""
  eps, kappa = 1.0 / beta, beta / (4.0 * T)
  var0 = 2.0 * (T + 1.0) / beta if var0 is None else var0
  x1 = np.asarray(x1, np.float64)
  x2 = x1 if x2 is None else np.asarray(x2, np.float64)
  ny, nw, y, _ = grids(dz, window, y_range)
  lg, logh = _log_h(beta, T, a, subtype, dz, window, y_range)
  Y1, Y2 = np.meshgrid(y, y)
  lr0 = _log_rho0(Y1, Y2, var0)
  r0 = np.exp(lr0)
  out = {"true_val": -2 * eps * np.sum(r0 * (logh - math.log(4 * math.pi * eps * T))) * dz * dz,
         "ic_mass": r0.sum() * dz * dz}
  L, m1, m2 = _to_outputs(lr0 - logh, y, x1, x2, kappa, True)
  _, m01, m02 = _to_outputs(lg[nw:nw + y.size, nw:nw + y.size], y, x1, x2, kappa, True)
  X1, X2 = np.meshgrid(x1, x2)
  return _finish(out, X1, X2, L, np.stack([m1, m2], -1), np.stack([m01, m02], -1), subtype, a, eps, T, dz)


def _lse(t, axis=-1):
  m = t.max(axis=axis, keepdims=True)
  return (m + np.log(np.exp(t - m).sum(axis=axis, keepdims=True))).squeeze(axis)


def direct(T, beta, a, subtype, x1, x2=None, var0=None, dz=0.2, window=6.0, y_range=4.0):
  """The generator's double sums point by point over the whole 2-D set (its loops at :117-123 and :171-186, each in
  log space): O(N^4), for coarse grids only."""
  eps, kappa = 1.0 / beta, beta / (4.0 * T)
  var0 = 2.0 * (T + 1.0) / beta if var0 is None else var0
  x1 = np.asarray(x1, np.float64)
  x2 = x1 if x2 is None else np.asarray(x2, np.float64)
  ny, nw, y, _ = grids(dz, window, y_range)
  off = np.arange(-nw, nw + 1)
  O1, O2 = [v.reshape(-1) for v in np.meshgrid(off, off)]
  Y1, Y2 = [v.reshape(-1) for v in np.meshgrid(y, y)]
  K1, K2 = [v.reshape(-1) for v in np.meshgrid(np.arange(-ny, ny + 1), np.arange(-ny, ny + 1))]
  logh = np.empty(Y1.size)
  for i in range(Y1.size):       # z = y + offset, by index
    z1, z2 = (K1[i] + O1) * dz, (K2[i] + O2) * dz
    logh[i] = _lse(-potential(z1, z2, subtype, a)[0] / (2 * eps) - kappa * ((O1 * dz) ** 2 + (O2 * dz) ** 2))
  logh += 2 * math.log(dz)
  lr0 = _log_rho0(Y1, Y2, var0)
  r0 = np.exp(lr0)
  out = {"true_val": -2 * eps * np.sum(r0 * (logh - math.log(4 * math.pi * eps * T))) * dz * dz,
         "ic_mass": r0.sum() * dz * dz}
  X1, X2 = np.meshgrid(x1, x2)
  gy = potential(Y1, Y2, subtype, a)[0]
  L = np.empty(X1.shape)
  m, m0 = np.empty(X1.shape + (2,)), np.empty(X1.shape + (2,))
  for idx in np.ndindex(X1.shape):
    d2 = (X1[idx] - Y1) ** 2 + (X2[idx] - Y2) ** 2
    t = lr0 - logh - kappa * d2
    L[idx] = _lse(t)
    w = np.exp(t - t.max())
    m[idx] = (w * Y1).sum() / w.sum(), (w * Y2).sum() / w.sum()
    t0 = -(gy + d2 / (2 * T)) / (2 * eps)
    w0 = np.exp(t0 - t0.max())
    m0[idx] = (w0 * Y1).sum() / w0.sum(), (w0 * Y2).sum() / w0.sum()
  return _finish(out, X1, X2, L, m, m0, subtype, a, eps, T, dz)


def closed_form(T, beta, s0, x1, x2=None):
  """The quadratic potential g = |x|^2 / 2 from N(0, s0 I), in the limit of unbounded ranges: rho_T = N(0, v_T I)
  with v_T = 1 / (2 (beta/4 + c gamma / (c + gamma))), c = beta / (4T), gamma = 1/(2 s0) - beta / (4 (T+1));
  score_T = -x / v_T, w0 = -x / (T+1) + eps x, wT = -x + eps x / v_T, true value 2 (eps log(T+1) + s0 / (2 (T+1)))."""
  eps = 1.0 / beta
  c, gam = beta / (4 * T), 1 / (2 * s0) - beta / (4 * (T + 1))
  vT = 1 / (2 * (beta / 4 + c * gam / (c + gam)))
  x1 = np.asarray(x1, np.float64)
  x2 = x1 if x2 is None else np.asarray(x2, np.float64)
  X1, X2 = np.meshgrid(x1, x2)
  x = np.stack([X1, X2], -1)
  return {"log_rho_T": -(X1 ** 2 + X2 ** 2) / (2 * vT) - math.log(2 * math.pi * vT), "score_T": -x / vT,
          "w0": -x / (T + 1) + eps * x, "wT": -x + eps * x / vT,
          "true_val": 2 * (eps * math.log(T + 1) + s0 / (2 * (T + 1)))}
