"""NumPy float64 restatement of cnf_rwpo_particles (include/cnf_ot_amd.h): the particle reference of the rwpo problems --
the Hopf-Cole formula read as an expectation, inner draws from a symmetric two-centre Gaussian proposal, one selected
endpoint per outer particle and a Brownian bridge to it.  It takes the flat normals (the cnf_fill_normal stream from
element first_particle * R on, or any normals laid out the same way) and the selection uniforms as arguments.  Test
infrastructure only.

The potentials are written out from applications.py:181-191 with the constants the loss kernels use (potential,
cnf_terms.h, the one definition on the device): `a` is a float32 value, widened.
"""
import math

import numpy as np

POTENTIALS = {"quadratic": 0, "double_well": 1, "obstacle": 2}


def stream_stride(D, K, S):
  """R: the stream elements a particle owns: D for y padded to a Philox block, per inner draw xi [D] and the sign normal
  padded to a block, then S D for the bridges, padded"""
  return 4 * (-(-D // 4) + K * (-(-(D + 1) // 4)) + -(-S * D // 4))


def particle_normals(flat, N, D, K, S):
  """flat -> (zy [N, D], xi [N, K, D], sign normal [N, K], zeta [N, S, D])"""
  R = stream_stride(D, K, S)
  by, bd = 4 * -(-D // 4), 4 * -(-(D + 1) // 4)
  z = np.asarray(flat, dtype=np.float64)[:N * R].reshape(N, R)
  draws = z[:, by:by + K * bd].reshape(N, K, bd)
  zeta = z[:, by + K * bd:by + K * bd + S * D].reshape(N, S, D)
  return z[:, :D], draws[:, :, :D], draws[:, :, D], zeta


def potential(z, subtype, a):
  """g(z) for z [..., D]"""
  a = float(np.float32(a))
  if subtype == "quadratic":
    return (z * z).sum(-1) * 0.5
  if subtype == "double_well":
    return ((z - a) ** 2).sum(-1) * ((z + a) ** 2).sum(-1) * 0.25
  if subtype == "obstacle":
    return np.exp((z * z).sum(-1) * -0.5) * 50.0
  raise ValueError(subtype)


def inner(y, xi, sign, subtype, a, T, beta, shrink, prop_var, centre=None):
  """The inner ensembles of the outer particles y [N, D] from xi [N, K, D] and the sign normals [N, K]: a dict of z
  [N, K, D], l [N, K], log_h, ess [N], mean_T [N, D] and L [N], the largest magnitude among the addends of any l_k"""
  N, K, D = xi.shape
  m = np.zeros(D) if centre is None else np.broadcast_to(np.asarray(centre, dtype=np.float64), (D,))
  sg = np.where(sign >= 0.0, 1.0, -1.0)
  mu = shrink * y
  z = (mu[:, None, :] + sg[:, :, None] * m) + math.sqrt(prop_var) * xi
  s2 = 2.0 * T / beta
  t_g = -beta * potential(z, subtype, a) / 2.0
  t_y = -((z - y[:, None, :]) ** 2).sum(-1) / (2.0 * s2)
  t_c = 0.5 * D * math.log(prop_var / s2)
  A = -((z - mu[:, None, :] - m) ** 2).sum(-1) / (2.0 * prop_var)
  B = -((z - mu[:, None, :] + m) ** 2).sum(-1) / (2.0 * prop_var)
  t_p = -np.logaddexp(A, B)
  l = t_g + t_y + t_c + t_p + math.log(2.0)
  L = np.max(np.maximum.reduce([np.abs(t_g), np.abs(t_y), np.full_like(t_g, abs(t_c)), np.abs(t_p)]), axis=1)
  mx = l.max(1)
  e = np.exp(l - mx[:, None])
  tot = e.sum(1)
  w = e / tot[:, None]
  return {"z": z, "l": l, "log_h": mx + np.log(tot) - math.log(K), "ess": 1.0 / (w * w).sum(1),
          "mean_T": (w[:, :, None] * z).sum(1), "L": L}


def select(l, u):
  """sel [N]: the smallest k whose cumulative sum of exp(l_j - max) over j <= k, ascending, exceeds u times the total
  (K - 1 if none does); gap [N]: the distance of u times the total from the nearest cumulative sum, over the total"""
  l = np.asarray(l, dtype=np.float64)
  u = np.asarray(u, dtype=np.float64)
  e = np.exp(l - l.max(1, keepdims=True))
  cum = np.cumsum(e, axis=1)
  tot = cum[:, -1]
  over = cum > (u * tot)[:, None]
  sel = np.where(over.any(1), over.argmax(1), l.shape[1] - 1)
  gap = np.abs(cum - (u * tot)[:, None]).min(1) / tot
  return sel.astype(np.int64), gap


def bridge(y, z_end, zeta, times, T, beta):
  """pos [S, N, D]: from (0, y) through the ascending times to (T, z_end), snapshot s driven by zeta [N, s, D];
  t = 0 gives y and t = T gives z_end exactly"""
  x, prev, out = np.array(y, dtype=np.float64), 0.0, []
  for s, t in enumerate(times):
    t = float(t)
    if t == T:
      x = np.array(z_end, dtype=np.float64)
    else:
      c = (t - prev) / (T - prev)
      sd = math.sqrt(2.0 / beta * (t - prev) * (T - t) / (T - prev))
      x = (x + c * (z_end - x)) + sd * zeta[:, s]
    out.append(x.copy())
    prev = t
  return np.stack(out)


def reference(flat, u, N, D, K, times, subtype, a, T, beta, var0, shrink, prop_var, centre=None):
  """Everything cnf_rwpo_particles returns per particle, from the flat normals and the uniforms u [N] (None: no
  selection and no path): inner()'s dict with y, and with u sel, gap, z_sel [N, D] and pos [S, N, D]"""
  S = len(times)
  zy, xi, sign, zeta = particle_normals(flat, N, D, K, S)
  y = math.sqrt(var0) * zy
  out = inner(y, xi, sign, subtype, a, T, beta, shrink, prop_var, centre)
  out["y"] = y
  if u is not None:
    out["sel"], out["gap"] = select(out["l"], u)
    out["z_sel"] = out["z"][np.arange(N), out["sel"]]
    out["pos"] = bridge(y, out["z_sel"], zeta, times, T, beta)
  return out


def value(log_h, ess, beta, K):
  """(true_val, true_val_se, bias_est, true_val_corrected)"""
  c = 2.0 / beta
  val = -c * log_h.mean()
  se = c * log_h.std(ddof=1) / math.sqrt(log_h.size)
  bias = c * ((1.0 / ess - 1.0 / K) / 2.0).mean()
  return val, se, bias, val - bias


def proposal(dim, T, beta, a, subtype):
  """applications.rwpo_proposal, restated"""
  if subtype == "quadratic":
    return dict(shrink=1.0 / (1.0 + T), prop_var=2.0 * T / (beta * (1.0 + T)), centre=None)
  if subtype == "double_well":
    P = beta * a * a * dim + beta / (2.0 * T)
    return dict(shrink=(beta / (2.0 * T)) / P, prop_var=1.0 / P, centre=np.full(dim, a * beta * a * a * dim / P))
  return dict(shrink=1.0, prop_var=2.0 * T / beta, centre=None)


def quadratic_log_h(y, T, beta):
  """log h(y) of the quadratic potential in closed form: -(D / 2) log(1 + T) - beta |y|^2 / (4 (1 + T))"""
  return -0.5 * y.shape[1] * math.log(1.0 + T) - beta * (y * y).sum(1) / (4.0 * (1.0 + T))
