"""float64 NumPy restatement of cnf_interaction_vjp and cnf_score_residual_force (include/cnf_ot_amd.h): the vector-
Jacobian product of the self-mode force f_i = (1 / (N - 1)) sum_{j != i} grad W(x_i - x_j) of interaction_ref,
  xbar_k = (1 / (N - 1)) sum_{j != k} H(x_k - x_j) (g_k - g_j),   H(d) v = c1 v + d (d . v) c2,
the pair Hessian's coefficients and its largest operator norm over a cloud's pairs (the scale of the GPU tests' floor),
the quadratic kind's closed form, and the score epilogue with strength * force inside the square.  Built on
interaction_ref and step_kernels_ref.  A helper: no tests in it.
"""
import numpy as np

import interaction_ref as ir
import step_kernels_ref as sk

CHUNK = 512


def hessian_coefficients(d2, sp):
  """(c1, c2) at the squared distances d2 (any shape): H(d) = c1 I + c2 d d^T; both 0 at distance 0 for the exponential
  kind (the force's own rule)"""
  d2 = np.asarray(d2, dtype=np.float64)
  if sp["kind"] == "quadratic":
    return np.full_like(d2, sp["amp"][0]), np.zeros_like(d2)
  c1, c2 = np.zeros_like(d2), np.zeros_like(d2)
  if sp["kind"] == "gaussian":
    for a, b in zip(sp["amp"], sp["bw"]):
      e = a * np.exp(-d2 / (2.0 * b * b))
      c1 -= e / (b * b)
      c2 += e / (b ** 4)
    return c1, c2
  r = np.sqrt(d2)
  ok = r > 0.0
  rs = np.where(ok, r, 1.0)
  w, wp = np.zeros_like(d2), np.zeros_like(d2)
  for a, b in zip(sp["amp"], sp["bw"]):
    e = a * np.exp(-r / b)
    w -= e / b
    wp += e / (b * b)
  return np.where(ok, w / rs, 0.0), np.where(ok, wp / rs ** 2 - w / rs ** 3, 0.0)


def force_vjp(x, g, sp):
  """xbar [N, D] for the points x [N, D] and the force's adjoint g [N, D], chunked over rows"""
  x, g = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
  N = len(x)
  out = np.empty_like(x)
  for i0 in range(0, N, CHUNK):
    diff = x[i0:i0 + CHUNK, None, :] - x[None, :, :]
    dv = g[i0:i0 + CHUNK, None, :] - g[None, :, :]
    c1, c2 = hessian_coefficients((diff * diff).sum(-1), sp)
    k = np.arange(diff.shape[0])
    c1[k, i0 + k] = 0.0                                      # (the pair j == k: dv is 0 there anyway)
    c2[k, i0 + k] = 0.0
    dot = (diff * dv).sum(-1)
    out[i0:i0 + CHUNK] = (c1[:, :, None] * dv + diff * (dot * c2)[:, :, None]).sum(1)
  return out / (N - 1.0)


def quadratic_closed_form(g, amp):
  """The quadratic kind: amp (N g_k - sum_j g_j) / (N - 1)"""
  g = np.asarray(g, dtype=np.float64)
  N = len(g)
  return amp * (N * g - g.sum(0)) / (N - 1.0)


def hessian_norm(x, sp):
  """eta: the largest operator norm of the pair Hessian over the cloud's pairs j != k, max(|c1|, |c1 + c2 d^2|) (the
  eigenvalues across and along d)"""
  x = np.asarray(x, dtype=np.float64)
  eta = 0.0
  for i0 in range(0, len(x), CHUNK):
    diff = x[i0:i0 + CHUNK, None, :] - x[None, :, :]
    d2 = (diff * diff).sum(-1)
    c1, c2 = hessian_coefficients(d2, sp)
    k = np.arange(diff.shape[0])
    c1[k, i0 + k] = 0.0
    c2[k, i0 + k] = 0.0
    eta = max(eta, float(np.abs(c1).max()), float(np.abs(c1 + c2 * d2).max()))
  return eta


def pair_spread(g):
  """max_{k, j} |g_k - g_j|, the Euclidean norm, over all pairs"""
  g = np.asarray(g, dtype=np.float64)
  best = 0.0
  for i0 in range(0, len(g), CHUNK):
    dv = g[i0:i0 + CHUNK, None, :] - g[None, :, :]
    best = max(best, float((dv * dv).sum(-1).max()))
  return float(np.sqrt(best))


def score_residual_force_ref(r, score, force, strength, n, count, D, dt, coef, drift, a, loss_coef):
  """(sums [ceil(n / count)], rbar [3 n, D], sbar [n, D], fbar [n, D]) of cnf_score_residual_force: score_residual_ref
  with u += strength force and fbar = strength u_bar"""
  r = np.asarray(r, dtype=np.float64).reshape(3 * n, D)
  u = sk.score_residual_u(r, score, n, D, dt, coef, drift, a) + strength * np.asarray(force, dtype=np.float64).reshape(n, D)
  ub = 2.0 * loss_coef * u
  rbar3 = -np.einsum("id,ide->ie", ub, sk.drift_jacobian(drift, r[2 * n:], a))
  return sk.slice_sums((u * u).sum(1), count), np.concatenate([-ub / dt, ub / dt, rbar3]), coef * ub, strength * ub
