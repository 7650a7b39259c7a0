"""Float64 numpy restatement of the 2-D Hopf-Cole solution at every time 0 <= t <= T (cnf_hopf_cole_path_2d), built on
hopf_cole_f64's passes, the direct O(N^4) sum at one time that pins it, and the quadratic potential's closed form.

With eps = 1/beta, lg = -g / (2 eps) on the whole z grid, H = log rho0 - log h on the y grid (h with its dz^2), and for
0 < t < T  kappa_b = 1 / (4 eps (T - t)), kappa_f = 1 / (4 eps t):
  log A_t(x) = LSE_z(lg(z) - kappa_b |x - z|^2) + 2 log dz - log(4 pi eps (T - t)),  m_b = the weighted mean of z
  log B_t(x) = LSE_y(H(y) - kappa_f |x - y|^2) + 2 log dz + log(T / t),              m_f = the weighted mean of y
  log_rho = log A + log B,  drift = -(x - m_b) / (T - t),  score = -(x - m_b) / (2 eps (T - t)) - (x - m_f) / (2 eps t),
  vel = drift - eps score
t = T: hopf_cole_f64.solve's log_rho_T, score_T, wT and drift = -grad g.  t = 0: log rho0, score = -x / var0,
drift = -(x - m0) / T with solve's m0 (w0 = drift + eps x), vel = drift + eps x / var0.
`solve` sums as two 1-D passes (the kernel's order), `direct` sums each point's whole 2-D set at once."""
import math

import numpy as np

import hopf_cole_f64 as hc

FIELDS = ("score", "drift", "vel")


def _xgrid(x1, x2):
  x1 = np.asarray(x1, np.float64)
  x2 = x1 if x2 is None else np.asarray(x2, np.float64)
  X1, X2 = np.meshgrid(x1, x2)
  return x1, x2, X1, X2, np.stack([X1, X2], -1)


def _to_outputs(lw, src, x1, x2, kappa):
  """hopf_cole_f64._to_outputs with the means, its row chunks sized to stay in cache (the z grid is 2.5 times the y
  grid per side): the same sums in the same order"""
  def free(lw, dst, carry):
    lk = -kappa * (dst[:, None] - src[None, :]) ** 2
    rows = max(1, 250000 // lk.size)
    return hc._lse_rows(hc._Terms(lw.shape[0], lambda r: lw[r, None, :] + lk), carry, src, chunk=rows)
  LC, MC, _ = free(lw, x1, None)                                   # [source 2, x1]
  L, M2, M1 = free(np.ascontiguousarray(LC.T), x2, np.ascontiguousarray(MC.T))   # [x1, x2]
  return L.T, M1.T, M2.T


def _endpoint(t, T, eps, var0, X1, X2, x, sol, subtype, a):
  """The slab at t = 0 or t = T from hopf_cole_f64's T solution `sol`"""
  if t == T:
    g = hc.potential(X1, X2, subtype, a)
    return {"log_rho": sol["log_rho_T"], "score": sol["score_T"], "vel": sol["wT"], "drift": -np.stack(g[1:], -1)}
  drift = sol["w0"] - eps * x
  return {"log_rho": hc._log_rho0(X1, X2, var0), "score": -x / var0, "drift": drift, "vel": drift + eps * x / var0}


def _interior(t, T, eps, dz, x, LA, mb, LB, mf):
  tb = T - t
  xb, xf = x - mb, x - mf
  drift = -xb / tb
  score = -xb / (2 * eps * tb) - xf / (2 * eps * t)
  return {"log_rho": (LA + 2 * math.log(dz) - math.log(4 * math.pi * eps * tb)) + (LB + 2 * math.log(dz) + math.log(T / t)),
          "score": score, "drift": drift, "vel": drift - eps * score}


def _stack(slabs, sol):
  out = {k: np.stack([s[k] for s in slabs]) for k in ("log_rho",) + FIELDS}
  out["true_val"], out["ic_mass"] = sol["true_val"], sol["ic_mass"]
  return out


def solve(T, beta, a, subtype, times, x1, x2=None, var0=None, dz=0.01, window=6.0, y_range=4.0):
  """The separable restatement: log_rho [S, n2, n1], score / drift / vel [S, n2, n1, 2], true_val, ic_mass."""
  eps = 1.0 / beta
  var0 = 2.0 * (T + 1.0) / beta if var0 is None else var0
  x1, x2, X1, X2, x = _xgrid(x1, x2)
  _, _, y, z = hc.grids(dz, window, y_range)
  lg, logh = hc._log_h(beta, T, a, subtype, dz, window, y_range)
  Y1, Y2 = np.meshgrid(y, y)
  H = hc._log_rho0(Y1, Y2, var0) - logh
  sol = hc.solve(T, beta, a, subtype, x1, x2, var0=var0, dz=dz, window=window, y_range=y_range)
  slabs = []
  for t in times:
    if t == 0 or t == T:
      slabs.append(_endpoint(t, T, eps, var0, X1, X2, x, sol, subtype, a))
      continue
    LA, b1, b2 = _to_outputs(lg, z, x1, x2, beta / (4.0 * (T - t)))
    LB, f1, f2 = _to_outputs(H, y, x1, x2, beta / (4.0 * t))
    slabs.append(_interior(t, T, eps, dz, x, LA, np.stack([b1, b2], -1), LB, np.stack([f1, f2], -1)))
  return _stack(slabs, sol)


def _direct_sum(lw, S1, S2, X1, X2, kappa):
  """LSE and weighted means of the flat source set (S1, S2) with log-weights lw, per output point"""
  L, m = np.empty(X1.shape), np.empty(X1.shape + (2,))
  for idx in np.ndindex(X1.shape):
    t = lw - kappa * ((X1[idx] - S1) ** 2 + (X2[idx] - S2) ** 2)
    L[idx] = hc._lse(t)
    w = np.exp(t - t.max())
    m[idx] = (w * S1).sum() / w.sum(), (w * S2).sum() / w.sum()
  return L, m


def direct(T, beta, a, subtype, times, x1, x2=None, var0=None, dz=0.2, window=6.0, y_range=4.0):
  """Every time's sums point by point over the whole 2-D source set, log h by hopf_cole_f64.direct's own double loop
  (recomputed here from its pieces): O(N^4), for coarse grids only."""
  eps, kappa = 1.0 / beta, beta / (4.0 * T)
  var0 = 2.0 * (T + 1.0) / beta if var0 is None else var0
  x1, x2, X1, X2, x = _xgrid(x1, x2)
  ny, nw, y, z = hc.grids(dz, window, y_range)
  off = np.arange(-nw, nw + 1)
  O1, O2 = [v.reshape(-1) for v in np.meshgrid(off, off)]
  Y1, Y2 = [v.reshape(-1) for v in np.meshgrid(y, y)]
  K1, K2 = [v.reshape(-1) for v in np.meshgrid(np.arange(-ny, ny + 1), np.arange(-ny, ny + 1))]
  Z1, Z2 = [v.reshape(-1) for v in np.meshgrid(z, z)]
  logh = np.empty(Y1.size)
  for i in range(Y1.size):
    z1, z2 = (K1[i] + O1) * dz, (K2[i] + O2) * dz
    logh[i] = hc._lse(-hc.potential(z1, z2, subtype, a)[0] / (2 * eps) - kappa * ((O1 * dz) ** 2 + (O2 * dz) ** 2))
  H = hc._log_rho0(Y1, Y2, var0) - (logh + 2 * math.log(dz))
  lg = -hc.potential(Z1, Z2, subtype, a)[0] / (2 * eps)
  sol = hc.direct(T, beta, a, subtype, x1, x2, var0=var0, dz=dz, window=window, y_range=y_range)
  slabs = []
  for t in times:
    if t == 0 or t == T:
      slabs.append(_endpoint(t, T, eps, var0, X1, X2, x, sol, subtype, a))
      continue
    LA, mb = _direct_sum(lg, Z1, Z2, X1, X2, beta / (4.0 * (T - t)))
    LB, mf = _direct_sum(H, Y1, Y2, X1, X2, beta / (4.0 * t))
    slabs.append(_interior(t, T, eps, dz, x, LA, mb, LB, mf))
  return _stack(slabs, sol)


def closed_form(T, beta, s0, times, x1, x2=None):
  """g = |x|^2 / 2 from N(0, s0 I) at unbounded ranges, u = 1 + T - t: rho_t = N(0, v_t I) with
  v_t = 2 eps u + (s0 - 2 eps (T + 1)) u^2 / (T + 1)^2, score = -x / v_t, drift = -x / u, vel = -x / u + eps x / v_t.
  At t = T it is hopf_cole_f64.closed_form."""
  eps = 1.0 / beta
  _, _, X1, X2, x = _xgrid(x1, x2)
  slabs = []
  for t in times:
    u = 1.0 + T - t
    v = 2 * eps * u + (s0 - 2 * eps * (T + 1)) * u * u / (T + 1) ** 2
    slabs.append({"log_rho": -(X1 ** 2 + X2 ** 2) / (2 * v) - math.log(2 * math.pi * v), "score": -x / v,
                  "drift": -x / u, "vel": -x / u + eps * x / v})
  return {k: np.stack([s[k] for s in slabs]) for k in ("log_rho",) + FIELDS}
