"""The float64 reference the exact score (cnf_score) is held to: central differences of oracle.log_prob at two steps,
and the rule that tells where such a difference means the derivative (test_input_adjoints_on_the_linear_tails' rule:
the spline is only C1, the score jumps at knots, and a difference that straddles one is off by O(1)).  Test helper: no
tests here, no GPU."""
import numpy as np

import oracle

CONDS = np.array([0.0, 0.35, 1.0], dtype=np.float32)       # the S = 3 slices of every case


def case_inputs(D, scale, seed, n=700):
  """(oracle config, float32 parameters N(0, scale^2), float32 points [3 n, D] from N(0, 1.5^2)) of one case; n = 700
  per slice is no multiple of 64 or of any tile."""
  ocfg = oracle.OracleConfig(D=D)
  rng = np.random.default_rng(seed)
  params = rng.normal(0.0, scale, oracle.param_count(ocfg)).astype(np.float32)
  pts = rng.normal(0.0, 1.5, (len(CONDS) * n, D)).astype(np.float32)
  return ocfg, params, pts


def fd_score(ocfg, params, pts, conds, h):
  """(log_prob(x + h e_d) - log_prob(x - h e_d)) / 2h in float64, [B, D]; conds: one value, or S values for S equal
  slices of pts."""
  p64, x = np.asarray(params, dtype=np.float64), np.asarray(pts, dtype=np.float64)
  c = np.asarray(conds, dtype=np.float64).reshape(-1)
  ref = np.empty_like(x)
  for d in range(x.shape[1]):
    xp, xm = x.copy(), x.copy()
    xp[:, d] += h
    xm[:, d] -= h
    ref[:, d] = (oracle.log_prob(ocfg, p64, xp, c) - oracle.log_prob(ocfg, p64, xm, c)) / (2 * h)
  return ref


def smooth_reference(ocfg, params, pts, conds, h=1e-6):
  """(ref [B, D] at step h, mag [B], smooth [B]): a point counts as smooth when the differences at h and 3 h agree to
  1e-3 mag, mag = max_d |ref| + 1e-3 median."""
  r1, r2 = fd_score(ocfg, params, pts, conds, h), fd_score(ocfg, params, pts, conds, 3 * h)
  top = np.abs(r1).max(1)
  mag = top + 1e-3 * np.median(top)
  return r1, mag, np.abs(r1 - r2).max(1) <= 1e-3 * mag
