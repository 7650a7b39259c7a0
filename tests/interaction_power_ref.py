"""float64 NumPy restatement of the power kind of cnf_interaction, cnf_interaction_vjp and cnf_mv_particles
(include/cnf_ot_amd.h), beside interaction_ref, interaction_vjp_ref and mv_particles_f64, whose other kinds it passes on:
with u = r^2 + eps^2,
  W(r) = sum_b amp_b u^(pw_b / 2) / pw_b  (pw_b != 0)  +  sum_b amp_b ln(u) / 2  (pw_b == 0),
  grad W = (x - y) w,  w = sum_b amp_b u^(pw_b / 2 - 1),
  H v = c1 v + d (d . v) c2,  c1 = w,  c2 = sum_b amp_b (pw_b - 2) u^(pw_b / 2 - 2);
the scales of the GPU tests' floors by the other kinds' rule, read over the pairs counted: k_max = sum_b max |W_b|,
tau = sum_b max |W_b'(r)| (interaction_ref's are these maxima in closed form), eta = the largest operator norm of the pair
Hessian (interaction_vjp_ref.hessian_norm's rule); the same sums composed in NumPy float32 throughout, the yardstick of
the fused error; and the log kernel's virial identity with its softening and Euler corrections.  A helper: no tests in it.

A spec is {"kind": "power", "amp": [...], "pw": [...], "eps": eps}.  At u = 0 (a coincident pair with eps = 0, every
pw_b >= 2) W = 0 and every weight with a negative power of u is 0, the kernel's rule.
"""
import numpy as np

import interaction_ref as ir
import interaction_vjp_ref as ivr
import mv_particles_f64 as mv

CHUNK = ir.CHUNK


def spec(pw, amp=None, eps=0.0):
  pw = [float(np.float32(p)) for p in pw]
  amp = [1.0] * len(pw) if amp is None else [float(np.float32(a)) for a in amp]
  assert len(amp) == len(pw)
  return {"kind": "power", "amp": amp, "pw": pw, "eps": float(np.float32(eps))}


def kwargs(sp):
  """The spec as utils.interaction_spec takes it"""
  if sp["kind"] != "power":
    return ir.kwargs(sp)
  return {"kind": "power", "amplitudes": sp["amp"], "bandwidths": sp["eps"] if sp["eps"] > 0.0 else None, "exponents": sp["pw"]}


def _upow(u, e):
  """u^e with 0^e = 0 for e < 0 as well (the coincident pair's rule) and 0^0 = 1"""
  if e >= 0.0:
    return u ** e
  ok = u > 0.0
  return np.where(ok, np.where(ok, u, 1.0) ** e, 0.0)


def terms(d2, sp, dtype=np.float64):
  """Per term b: (W_b, w_b, c2_b) at the squared distances d2, in `dtype` throughout"""
  f = dtype
  u = d2.astype(f) + f(sp["eps"]) * f(sp["eps"])
  out = []
  for a, p in zip(sp["amp"], sp["pw"]):
    a, h = f(a), f(0.5 * p)
    if p == 0.0:
      with np.errstate(divide="ignore"):      # (the pair i == i of a cloud with eps = 0: left out by index afterwards)
        W = f(0.5) * a * np.log(u)
    else:
      W = (a / f(p)) * u ** h
    out.append((W.astype(f), (a * _upow(u, h - f(1.0))).astype(f), (a * f(p - 2.0) * _upow(u, h - f(2.0))).astype(f)))
  return out


def kernel(diff, sp, dtype=np.float64):
  """(W, w) [r, c] for differences diff [r, c, D]"""
  if sp["kind"] != "power":
    assert dtype == np.float64
    return ir._kernel(diff, sp)
  t = terms((diff * diff).sum(-1, dtype=dtype), sp, dtype)
  return sum(x[0] for x in t), sum(x[1] for x in t)


def rows(x, sp, q=None, dtype=np.float64):
  """interaction_ref.rows for every kind: (pot [rows], force [rows, D], raw sum, None); dtype float32 composes the
  differences, distances, the kernel, the products and the sums over the columns in float32 throughout"""
  if sp["kind"] != "power" and dtype == np.float64:
    return ir.rows(x, sp, q)
  x = np.asarray(x, dtype=dtype)
  self_mode = q is None
  a = x if self_mode else np.asarray(q, dtype=dtype)
  n = len(x) - 1 if self_mode else len(x)
  pot, force = np.empty(len(a), dtype=dtype), np.empty_like(a)
  for i0 in range(0, len(a), CHUNK):
    diff = a[i0:i0 + CHUNK, None, :] - x[None, :, :]
    W, w = kernel(diff, sp, dtype)
    if self_mode:
      r = np.arange(len(W))
      W[r, i0 + r] = 0
      w[r, i0 + r] = 0
    assert W.dtype == w.dtype == diff.dtype == dtype
    pot[i0:i0 + CHUNK] = W.sum(1, dtype=dtype)
    force[i0:i0 + CHUNK] = (diff * w[:, :, None]).sum(1, dtype=dtype)
  total = float(pot.astype(np.float64).sum())
  return (pot / dtype(n)).astype(np.float64), (force / dtype(n)).astype(np.float64), total, None


def scales(x, sp, q=None):
  """(k_max, tau, eta) over the pairs counted (self mode: j != i)"""
  if sp["kind"] != "power":
    return ir.k_max(x, sp, q), ir.tau(x, sp, q), (ivr.hessian_norm(x, sp) if q is None else None)
  x = np.asarray(x, dtype=np.float64)
  a = x if q is None else np.asarray(q, dtype=np.float64)
  nb = len(sp["pw"])
  kb, tb, eta = np.zeros(nb), np.zeros(nb), 0.0
  for i0 in range(0, len(a), CHUNK):
    diff = a[i0:i0 + CHUNK, None, :] - x[None, :, :]
    d2 = (diff * diff).sum(-1)
    keep = np.ones_like(d2, dtype=bool)
    if q is None:
      r = np.arange(len(d2))
      keep[r, i0 + r] = False
    t = terms(d2, sp)
    for b, (W, w, _) in enumerate(t):
      kb[b] = max(kb[b], float(np.abs(W[keep]).max()))
      tb[b] = max(tb[b], float((np.abs(w) * np.sqrt(d2))[keep].max()))
    c1, c2 = sum(v[1] for v in t), sum(v[2] for v in t)
    eta = max(eta, float(np.abs(c1[keep]).max()), float(np.abs(c1 + c2 * d2)[keep].max()))
  return float(kb.sum()), float(tb.sum()), eta


def hessian_coefficients(d2, sp, dtype=np.float64):
  if sp["kind"] != "power":
    return ivr.hessian_coefficients(d2, sp)
  t = terms(np.asarray(d2), sp, dtype)
  return sum(v[1] for v in t), sum(v[2] for v in t)


def force_vjp(x, g, sp, dtype=np.float64):
  """interaction_vjp_ref.force_vjp for every kind; dtype float32: composed in float32 throughout"""
  if sp["kind"] != "power" and dtype == np.float64:
    return ivr.force_vjp(x, g, sp)
  x, g = np.asarray(x, dtype=dtype), np.asarray(g, dtype=dtype)
  N = len(x)
  out = np.empty_like(x)
  for i0 in range(0, N, CHUNK):
    diff = x[i0:i0 + CHUNK, None, :] - x[None, :, :]
    dv = g[i0:i0 + CHUNK, None, :] - g[None, :, :]
    c1, c2 = hessian_coefficients((diff * diff).sum(-1, dtype=dtype), sp, dtype)
    k = np.arange(diff.shape[0])
    c1[k, i0 + k] = 0
    c2[k, i0 + k] = 0
    dot = (diff * dv).sum(-1, dtype=dtype)
    res = (c1[:, :, None] * dv + diff * (dot * c2)[:, :, None])
    assert res.dtype == dtype
    out[i0:i0 + CHUNK] = res.sum(1, dtype=dtype)
  return (out / dtype(N - 1)).astype(np.float64)


def force_f64(x, sp):
  """mv_particles_f64.force_f64 for every kind"""
  _, G, total, _ = rows(mv.rounded(x), sp)
  return G, total


def force_f32(x, sp):
  """mv_particles_f64.force_f32 for every kind"""
  if sp["kind"] != "power":
    return mv.force_f32(x, sp)
  _, G, total, _ = rows(np.asarray(x, dtype=np.float64).astype(np.float32), sp, dtype=np.float32)
  return G, total


def energy(x, sp):
  N = len(x)
  return rows(x, sp)[2] / (2.0 * N * (N - 1.0))


def quadratic_restatement(diff, amp):
  """interaction_ref's quadratic kind on the same differences: (W, w)"""
  return ir._kernel(diff, ir.spec("quadratic", [amp]))


# ---- the log kernel's virial identity ---------------------------------------------------------------------------------

def virial_sum(x, sp):
  """sum_i x_i . f_i with f_i = mean_{j != i} grad W(x_i - x_j): amp N / 2 for the log kernel with eps = 0"""
  x = np.asarray(x, dtype=np.float64)
  return float((x * rows(x, sp)[1]).sum())


def log_second_moment_increments(z, sigma, h, var0, kappa, sp, steps, x0=None, force=force_f64):
  """The restatement's path of R replicas from normals z [R, N, steps + 1, D] with no drift, and what its mean |x|^2 owes
  to each cause: returns (m2 [steps + 1, R] = mean_i |x_i|^2 per step and replica, expected [R]: the sum over the steps
  of the CONDITIONAL expectation of the increment of mean |x|^2 given the positions,
      -2 h kappa mean_i x_i . G_i + h^2 kappa^2 mean_i |G_i|^2 + 2 D sigma h,
  which holds the softening (x . G is the pair mean of amp d^2 / (d^2 + eps^2), not amp) and the Euler term exactly, and
  per_particle [R, N]: each particle's total increment minus its own conditional expectation, whose standard deviation
  over the particles gives the standard error of the mean's martingale part)"""
  z = np.asarray(z, dtype=np.float64)
  R, N, _, D = z.shape
  x = np.sqrt(var0) * z[:, :, 0] if x0 is None else np.array(x0, dtype=np.float64)
  sdn = np.sqrt(2.0 * sigma * h)
  m2, expected, resid = [(x * x).sum(-1).mean(1)], np.zeros(R), np.zeros((R, N))
  for k in range(steps):
    G = np.stack([force(x[r], sp)[0] for r in range(R)])
    cond = -2.0 * h * kappa * (x * G).sum(-1) + h * h * kappa * kappa * (G * G).sum(-1) + 2.0 * D * sigma * h
    xn = (x + h * (-kappa * G)) + sdn * z[:, :, k + 1]
    resid += (xn * xn).sum(-1) - (x * x).sum(-1) - cond
    expected += cond.mean(1)
    x = xn
    m2.append((x * x).sum(-1).mean(1))
  return np.asarray(m2), expected, resid


def cloud(D, N, seed, scale=1.2, S=None):
  return ir.cloud(D, N, seed, scale, S)
