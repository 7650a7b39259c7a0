"""Float64 reference of the importance-sampling diagnostics (cnf_importance_stats, applications.importance_stats),
shared by test_importance_cpu and test_gpu_importance.  Test helpers only: no tests here.

The flow's samples and log-density come from the CPU oracle on given base noise; the target's log-density is
restated here in NumPy from the target's own means / covariance (not from the packed whitening matrix the kernel
reads); the raw state (m, s1, s2, c, n) and the derived numbers go through scipy.special.logsumexp.  `naive` is
the reference's own linear-space arithmetic (tests/test_fit_prob.py:50-56), kept to show where it underflows.
"""
import numpy as np
from scipy.special import logsumexp


def target_logprob(means, cov, log_weights, y, scale=1.0):
  """log sum_m w_m N(y; mu_m, scale * cov) for y [n, D], float64."""
  means = np.atleast_2d(np.asarray(means, dtype=np.float64))
  y = np.asarray(y, dtype=np.float64)
  D = y.shape[1]
  cov = np.eye(D) if cov is None else (float(cov) * np.eye(D) if np.ndim(cov) == 0 else np.asarray(cov, dtype=np.float64))
  prec = np.linalg.inv(cov)
  _, logdet = np.linalg.slogdet(cov)
  diff = y[:, None, :] - means[None, :, :]                        # [n, M, D]
  q = np.einsum("nmd,de,nme->nm", diff, prec, diff) / scale
  lw = np.full(means.shape[0], -np.log(means.shape[0])) if log_weights is None else np.asarray(log_weights, dtype=np.float64)
  return logsumexp(lw[None, :] - 0.5 * q, axis=1) - 0.5 * D * np.log(2.0 * np.pi * scale) - 0.5 * logdet


def raw_state(logw):
  """(m, s1, s2, c, n) of one slice's log-weights"""
  logw = np.asarray(logw, dtype=np.float64)
  if logw.size == 0:
    return np.array([-np.inf, 0.0, 0.0, 0.0, 0.0])
  m = logw.max()
  return np.array([m, np.exp(logsumexp(logw - m)), np.exp(logsumexp(2.0 * (logw - m))), logw.sum(), float(logw.size)])


def summary(logw):
  """log_Z, KL, ess of one slice's log-weights, in log space"""
  logw = np.asarray(logw, dtype=np.float64)
  n = logw.size
  log_Z = logsumexp(logw) - np.log(n)
  return {"log_Z": log_Z, "KL": -logw.mean() + log_Z, "ess": np.exp(2.0 * logsumexp(logw) - logsumexp(2.0 * logw)),
          "max_log_w": logw.max(), "n": n}


def summary_of_raw(raw):
  """the same numbers from a raw [5] state (what applications.importance_summary computes)"""
  m, s1, s2, c, n = [float(v) for v in raw]
  log_Z = np.log(s1) + m - np.log(n)
  return {"log_Z": log_Z, "KL": -c / n + log_Z, "ess": np.exp(2.0 * np.log(s1) - np.log(s2)), "max_log_w": m, "n": n}


def naive(log_p, log_q):
  """kl_ess as the reference writes it: w = p / exp(log q) in linear space"""
  with np.errstate(all="ignore"):
    w = np.exp(log_p) / np.exp(log_q)
    Z = w.mean()
    return {"Z": Z, "KL": np.mean(log_q - log_p) + np.log(Z), "ess": w.sum() ** 2 / (w ** 2).sum()}


def log_weights(target, y, log_q, scale=1.0):
  """l = log p_target(y) - log q for a cnf_ot_amd.applications.GaussianMixtureTarget"""
  return target_logprob(target.means, target.cov, target.log_weights, y, scale) - np.asarray(log_q, dtype=np.float64)


def oracle_log_weights(oracle, ocfg, params64, noise, conds, target, scales=None):
  """Per slice of `conds`: (log-weights [B], oracle samples [B, D], oracle log_prob [B]) in float64, noise
  [S * B, D] (slice s = rows [s B, (s + 1) B))."""
  noise = np.asarray(noise, dtype=np.float64)
  S = len(conds)
  B = noise.shape[0] // S
  out = []
  for s in range(S):
    y, lq = oracle.sample_logprob(ocfg, params64, noise[s * B:(s + 1) * B], [float(conds[s])])
    sc = 1.0 if scales is None else float(scales[s])
    out.append((log_weights(target, y, lq, sc), y, lq))
  return out
