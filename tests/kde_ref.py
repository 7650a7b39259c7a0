"""The Gaussian kernel density estimate of cnf_kde restated in NumPy: float64 is the reference of tests/test_gpu_kde.py
and tests/test_kde_cpu.py, and the same composition in float32 (t and exp(t - m) in float32, reduced in float64) gives
the e_composed of the project's bar  e_fused <= 2 e_composed + 4 EPS scale.

Sources x [N, D], queries q [Q, D] (None: the sources), bandwidth h:
  t_ij     = -|q_i - x_j|^2 / (2 h^2)            (the difference first, then the square)
  m        = max_j t_ij,   s = sum_j exp(t_ij - m),   w_ij = exp(t_ij - m) / s
  log_rho  = m + log s - log n_eff - (D / 2) log(2 pi h^2)
  score_d  = sum_j w_ij (x_jd - q_id) / h^2
  loo (self mode): the pair j == i is skipped by index, n_eff = N - 1; else n_eff = N
  a row whose every t_ij is -inf: log_rho = -inf, score = 0
"""
import numpy as np


def bandwidths(bws):
  return [float(np.float32(b)) for b in bws]      # (as the kernel receives them)


def cloud(D, N, seed, scale=1.0, shift=0.0):
  rng = np.random.default_rng(seed)
  return (scale * rng.standard_normal((N, D)) + shift).astype(np.float32)


def kde(x, q, h, loo=False, dtype=np.float64, chunk=256):
  """ONE set and ONE bandwidth: a dict of log_rho [Q], score [Q, D], m [Q] (each row's largest t) and absw [Q, D] =
  sum_j w_ij |x_jd - q_id| / h^2 (the scale of the score's bar), float64 arrays; the pair quantities t and exp(t - m)
  are formed in dtype and reduced in float64.  Rows are chunked so that no Q x N x D array is held."""
  x = np.asarray(x, dtype=dtype)
  self_mode = q is None
  q = x if self_mode else np.asarray(q, dtype=dtype)
  assert self_mode or not loo
  N, D = x.shape
  Q = q.shape[0]
  h = float(np.float32(h))
  log_rho, m_all = np.zeros(Q), np.zeros(Q)
  score, absw = np.zeros((Q, D)), np.zeros((Q, D))
  n_eff = N - 1 if loo else N
  cst = -np.log(float(n_eff)) - 0.5 * D * np.log(2.0 * np.pi * h * h)
  with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
    for i0 in range(0, Q, chunk):
      qi = q[i0:i0 + chunk]
      d = x[None, :, :] - qi[:, None, :]           # x_j - q_i
      d2 = (d * d).sum(-1)
      t = -d2 / dtype(2.0 * h * h)
      if loo:
        k = np.arange(len(qi))
        t[k, i0 + k] = -np.inf                     # the pair i == j, by index
      m = t.max(1)
      dead = np.isneginf(m)
      e = np.exp(t - np.where(dead, dtype(0.0), m)[:, None])      # (a dead row: exp(-inf) = 0, not exp(nan))
      e64 = e.astype(np.float64)
      s = e64.sum(1)
      w = e64 / np.where(dead, 1.0, s)[:, None]
      d64 = d.astype(np.float64)
      log_rho[i0:i0 + chunk] = np.where(dead, -np.inf, m.astype(np.float64) + np.log(np.where(dead, 1.0, s)) + cst)
      with np.errstate(all="ignore"):
        sc = np.where(w[:, :, None] == 0.0, 0.0, w[:, :, None] * d64).sum(1) / (h * h)
        ab = np.where(w[:, :, None] == 0.0, 0.0, w[:, :, None] * np.abs(d64)).sum(1) / (h * h)
      score[i0:i0 + chunk] = np.where(dead[:, None], 0.0, sc)
      absw[i0:i0 + chunk] = np.where(dead[:, None], 0.0, ab)
      m_all[i0:i0 + chunk] = m
  return {"log_rho": log_rho, "score": score, "m": m_all, "absw": absw}


def normal_pdf(q, var):
  """N(q; 0, var I) at the rows of q, float64"""
  q = np.asarray(q, dtype=np.float64)
  D = q.shape[-1]
  return np.exp(-0.5 * (q * q).sum(-1) / var) / (2.0 * np.pi * var) ** (0.5 * D)
