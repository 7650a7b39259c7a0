"""float64 NumPy restatement of the kernel two-sample statistics of cnf_mmd2 (include/cnf_ot_amd.h): the raw pair sums,
the unbiased MMD^2 / energy distance and its gradient in x, chunked over rows so that 4 000 x 4 000 pairs fit, and the
closed form of a Gaussian kernel's population mean between two isotropic Gaussians.  A helper: no tests in it.

A spec is {"kind": "gaussian", "bw": [...]} or {"kind": "energy"}.
"""
import numpy as np

CHUNK = 512


def spec(kind, bw=()):
  return {"kind": kind, "bw": [float(b) for b in bw]}


def _kernel(diff, sp):
  """k [r, c] and the weight w [r, c] with d k / d (first argument) = -diff w, for differences diff [r, c, D]"""
  d2 = (diff * diff).sum(-1)
  if sp["kind"] == "energy":
    d = np.sqrt(d2)
    with np.errstate(divide="ignore"):
      w = np.where(d > 0.0, 1.0 / np.where(d > 0.0, d, 1.0), 0.0)
    return -d, w
  k = np.zeros_like(d2)
  w = np.zeros_like(d2)
  for bw in sp["bw"]:
    e = np.exp(-d2 / (2.0 * bw * bw))
    k += e
    w += e / (bw * bw)
  return k, w


def _block(a, b, sp, skip_diag, want_grad=False):
  """(sum over pairs of k(a_i, b_j), the rows' sum_j d k(a_i, b_j) / d a_i or None, the largest |k|); skip_diag
  leaves i == j out by index"""
  a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
  total, kmax = 0.0, 0.0
  g = np.zeros_like(a) if want_grad else None
  for i0 in range(0, len(a), CHUNK):
    diff = a[i0:i0 + CHUNK, None, :] - b[None, :, :]
    k, w = _kernel(diff, sp)
    if skip_diag:
      r = np.arange(len(k))
      k[r, i0 + r] = 0.0
      w[r, i0 + r] = 0.0
    total += k.sum()
    kmax = max(kmax, float(np.abs(k).max()))
    if want_grad:
      g[i0:i0 + CHUNK] = -(diff * w[:, :, None]).sum(1)
  return total, g, kmax


def row_means(a, b, sp, skip_diag):
  """mean_j k(a_i, b_j) per row i (skip_diag: over j != i) -- what the standard error of a pair mean is read from"""
  a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
  out = np.empty(len(a))
  for i0 in range(0, len(a), CHUNK):
    k, _ = _kernel(a[i0:i0 + CHUNK, None, :] - b[None, :, :], sp)
    if skip_diag:
      r = np.arange(len(k))
      k[r, i0 + r] = 0.0
    out[i0:i0 + CHUNK] = k.sum(1) / (len(b) - (1 if skip_diag else 0))
  return out


def sums(x, y, sp):
  """(sxx, syy, sxy): sum_{i != j} k(x_i, x_j), sum_{i != j} k(y_i, y_j), sum_{i, j} k(x_i, y_j)"""
  return np.array([_block(x, x, sp, True)[0], _block(y, y, sp, True)[0], _block(x, y, sp, False)[0]])


def mmd2_of_sums(s, N, M):
  return s[0] / (N * (N - 1.0)) + s[1] / (M * (M - 1.0)) - 2.0 * s[2] / (float(N) * M)


def mmd2(x, y, sp):
  return mmd2_of_sums(sums(x, y, sp), len(x), len(y))


def xgrad(x, y, sp):
  """d mmd2 / d x [N, D]: (2 / (N (N - 1))) sum_{j != i} d k(x_i, x_j) / d x_i - (2 / (N M)) sum_j d k(x_i, y_j) / d x_i"""
  N, M = len(x), len(y)
  return 2.0 / (N * (N - 1.0)) * _block(x, x, sp, True, True)[1] - 2.0 / (float(N) * M) * _block(x, y, sp, False, True)[1]


def k_max(x, y, sp):
  """The scale of the value's floor: n_bw for the Gaussian sum, the largest pair distance for the energy kernel"""
  if sp["kind"] == "gaussian":
    return float(len(sp["bw"]))
  return max(_block(x, x, sp, True)[2], _block(y, y, sp, True)[2], _block(x, y, sp, False)[2])


def tau(sp):
  """The scale of the gradient's floor: sum_b max_r (r / bw^2) exp(-r^2 / (2 bw^2)) = sum_b 0.61 / bw_b; 1 for energy"""
  return sum(0.61 / bw for bw in sp["bw"]) if sp["kind"] == "gaussian" else 1.0


def population_gaussian(D, mu, s1, s2, bw):
  """E exp(-|x - y|^2 / (2 bw^2)) for x ~ N(0, s1^2 I_D), y ~ N(m, s2^2 I_D) with |m| = mu (s1 = s2, mu = 0: both
  from one law): (bw^2 / (bw^2 + s1^2 + s2^2))^(D / 2) exp(-mu^2 / (2 (bw^2 + s1^2 + s2^2)))"""
  v = bw * bw + s1 * s1 + s2 * s2
  return (bw * bw / v) ** (D / 2.0) * np.exp(-mu * mu / (2.0 * v))


def population_mmd2(D, mu, s1, s2, bws):
  """The population MMD^2 between N(0, s1^2 I) and N(m, s2^2 I) under the Gaussian sum kernel"""
  return sum(population_gaussian(D, 0.0, s1, s1, b) + population_gaussian(D, 0.0, s2, s2, b)
             - 2.0 * population_gaussian(D, mu, s1, s2, b) for b in bws)


def clouds(D, N, M, seed, shift=0.3, scale=1.2, S=None):
  """The tests' inputs: x ~ N(0, I), y ~ N(shift (1, ..., 1), scale^2 I), rounded to float32 ([S, ., D] with S)"""
  rng = np.random.default_rng(seed)
  lead = () if S is None else (S,)
  x = rng.standard_normal(lead + (N, D)).astype(np.float32)
  y = (shift + scale * rng.standard_normal(lead + (M, D))).astype(np.float32)
  return x, y
