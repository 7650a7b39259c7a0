"""float64 NumPy restatement of cnf_interaction (include/cnf_ot_amd.h): the raw double sum, the field (W * rho)(row_i),
the force grad (W * rho)(row_i), the energy F and dF / dx, in self mode (q None: the pair i == j left out by index) and
in query mode, chunked over rows; the scales k_max and tau of the GPU tests' floors; and the closed forms the restatement
is pinned against.  A helper: no tests in it.

A spec is {"kind": "gaussian" | "exponential" | "quadratic", "amp": [...], "bw": [...]}; W(r) as the header states it.
"""
import math

import numpy as np

CHUNK = 512


def spec(kind, amp=(1.0,), bw=(1.0,)):
  if kind == "quadratic":
    return {"kind": kind, "amp": [float(amp[0])], "bw": []}
  assert len(amp) == len(bw)
  return {"kind": kind, "amp": [float(a) for a in amp], "bw": [float(b) for b in bw]}


def kwargs(sp):
  """The spec as utils.interaction_spec takes it"""
  return {"kind": sp["kind"], "amplitudes": sp["amp"], "bandwidths": sp["bw"] or None}


def _kernel(diff, sp):
  """W [r, c] and the weight w [r, c] with grad W = diff w, for differences diff [r, c, D] (w = 0 at distance 0 for the
  exponential kind)"""
  d2 = (diff * diff).sum(-1)
  if sp["kind"] == "quadratic":
    return 0.5 * sp["amp"][0] * d2, np.full_like(d2, sp["amp"][0])
  W, w = np.zeros_like(d2), np.zeros_like(d2)
  if sp["kind"] == "gaussian":
    for a, b in zip(sp["amp"], sp["bw"]):
      e = a * np.exp(-d2 / (2.0 * b * b))
      W += e
      w -= e / (b * b)
    return W, w
  r = np.sqrt(d2)
  inv = np.where(r > 0.0, 1.0 / np.where(r > 0.0, r, 1.0), 0.0)
  for a, b in zip(sp["amp"], sp["bw"]):
    e = a * np.exp(-r / b)
    W += e
    w -= e / b * inv
  return W, w


def rows(x, sp, q=None):
  """(pot [rows], force [rows, D], raw sum, the largest d^2 over the pairs counted): pot and force are means over
  n = N - 1 (self mode, q None) or N (query mode) sources"""
  x = np.asarray(x, dtype=np.float64)
  self_mode = q is None
  a = x if self_mode else np.asarray(q, dtype=np.float64)
  n = len(x) - 1 if self_mode else len(x)
  pot, force, d2max = np.empty(len(a)), np.empty_like(a), 0.0
  for i0 in range(0, len(a), CHUNK):
    diff = a[i0:i0 + CHUNK, None, :] - x[None, :, :]
    W, w = _kernel(diff, sp)
    if self_mode:
      r = np.arange(len(W))
      W[r, i0 + r] = 0.0
      w[r, i0 + r] = 0.0
    pot[i0:i0 + CHUNK] = W.sum(1)
    force[i0:i0 + CHUNK] = (diff * w[:, :, None]).sum(1)
    d2max = max(d2max, float((diff * diff).sum(-1).max()))
  return pot / n, force / n, float(pot.sum()), d2max


def sums(x, sp, q=None):
  return rows(x, sp, q)[2]


def potential(x, sp, q=None):
  return rows(x, sp, q)[0]


def force(x, sp, q=None):
  return rows(x, sp, q)[1]


def energy(x, sp):
  """F = sum_{i != j} W / (2 N (N - 1))"""
  N = len(x)
  return sums(x, sp) / (2.0 * N * (N - 1.0))


def xgrad(x, sp):
  """dF / dx [N, D] = force / N (W is even)"""
  return force(x, sp) / len(x)


def k_max(x, sp, q=None):
  """The scale of the value's floor: sum_b |amp_b|, or |amp_0| max d^2 / 2 for the quadratic kind"""
  if sp["kind"] == "quadratic":
    return abs(sp["amp"][0]) * rows(x, sp, q)[3] / 2.0
  return sum(abs(a) for a in sp["amp"])


def tau(x, sp, q=None):
  """The scale of the force's floor: sum_b |amp_b| max_r |W_b'(r)| = 0.61 / bw_b (Gaussian: (r / bw^2) exp(-r^2 / (2
  bw^2)) at r = bw is exp(-1/2) / bw) or 1 / bw_b (exponential); |amp_0| times the largest pair distance (quadratic)"""
  if sp["kind"] == "quadratic":
    return abs(sp["amp"][0]) * math.sqrt(rows(x, sp, q)[3])
  return sum(abs(a) * (0.61 if sp["kind"] == "gaussian" else 1.0) / b for a, b in zip(sp["amp"], sp["bw"]))


def row_means(x, sp):
  """mean_{j != i} W(x_i - x_j) per row: what the standard error of the pair mean is read from"""
  return potential(x, sp)


def population_gaussian(D, s, bw):
  """E exp(-|x - y|^2 / (2 bw^2)) for x, y ~ N(0, s^2 I_D) independent: (bw^2 / (bw^2 + 2 s^2))^(D / 2)"""
  return (bw * bw / (bw * bw + 2.0 * s * s)) ** (D / 2.0)


def population_exponential_1d(s, bw):
  """E exp(-|x - y| / bw) for x, y ~ N(0, s^2) independent: x - y ~ N(0, tau^2), tau^2 = 2 s^2, and
  E exp(-|u| / bw) = exp(tau^2 / (2 bw^2)) erfc(tau / (sqrt 2 bw))"""
  t = math.sqrt(2.0) * s
  return math.exp(t * t / (2.0 * bw * bw)) * math.erfc(t / (math.sqrt(2.0) * bw))


def cloud(D, N, seed, scale=1.2, S=None):
  """The tests' inputs: scale * N(0, I), rounded to float32 ([S, N, D] with S)"""
  lead = () if S is None else (S,)
  return (np.random.default_rng(seed).standard_normal(lead + (N, D)) * scale).astype(np.float32)
